"""PBR under PCSS on the GPU (shs_rt_render_pbr_soft, shs_rt_frame::shading 3: PASS1 of hello_pbr_light_shafts.cpp) against
tests/canvas_rt_pbr_soft_ref (test_canvas_rt_pbr_soft_ref.py holds the wrapper, the frames and what pins the reference on
the CPU; the scenes, materials and IBLs are test_canvas_rt_pbr_ref's, the PCSS constants test_canvas_rt_soft_ref's).

Per frame, on every pixel, none excused (check_camera_soft): the view-z depth, the velocity and the PCSS factor (the
prequant plane's alpha) bit-exact; the shading sub-triangle and the setup counters equal; colours through
helpers.assert_color_parity with the pre-truncation floats within helpers.TOL * 255.  PASS0 is the hard demo's and is
compared as there.

The texel a textured pixel samples: the sampling code is shading 2's, whose tests read the texel back on every pixel.
Here it is pinned by sensitivity -- test_texel_identity renders the frame test_canvas_rt_pbr_soft_ref.texel_frame, on which
the restatement shows that any neighbouring texel would move a channel by more than ten times the bar."""
import ctypes
import dataclasses

import numpy as np
import pytest

import helpers
import test_canvas_light_shafts as LS
import test_canvas_light_shafts_ref as L
import test_canvas_rt as T
import test_canvas_rt_pbr_ref as P
import test_canvas_rt_pbr_soft_ref as Q
import test_canvas_rt_ref as R
import test_canvas_rt_sky_ref as K
import test_canvas_rt_soft_ref as S
from test_canvas_rt_ref import F, H, SM, W

pytestmark = pytest.mark.gpu
IBL = P.make_ibl()          # irradiance 4^2, specular 8, 4, 2, 1


@pytest.fixture(scope="module")
def ctx():
    import shs_gpu
    c = shs_gpu.Context(0)
    yield c
    c.close()


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _set(c, ibl, consts, pcss):
    if ibl is None:
        c.rt_set_ibl(None)
    else:
        c.rt_set_ibl(*ibl)
    c.rt_set_pbr(consts)
    c.rt_set_pcss(pcss)


def compare_planes(color, depth, vel, pq, ids, ref, label):
    helpers.assert_depth_bitexact(depth, ref["depth"])
    bad = np.argwhere(ids != ref["tri_id"])
    assert bad.size == 0, f"{len(bad)} pixels shaded by another sub-triangle, first {bad[:4].tolist()}"
    bad = np.argwhere((_bits(vel) != _bits(ref["velocity"])).any(-1))
    assert bad.size == 0, f"{len(bad)} velocities differ, first {bad[:4].tolist()}"
    bad = np.argwhere(_bits(pq[..., 3]) != _bits(ref["prequant"][..., 3]))
    assert bad.size == 0, f"{len(bad)} PCSS factors differ, first {bad[:4].tolist()}"
    n = helpers.assert_color_parity(color, ref["color"], pq, ref["prequant"])
    dp = np.abs(pq[..., :3] - ref["prequant"][..., :3])
    exact = int((_bits(pq[..., :3]) != _bits(ref["prequant"][..., :3])).sum())
    print(f"{label}: {exact} of {3 * int((ids >= 0).sum())} colour floats not bit-identical, {n} bytes off by one, "
          f"max float difference {dp.max():.3g} (bar {helpers.TOL * 255:.3g})")
    assert dp.max() <= helpers.TOL * 255.0, f"pre-truncation floats differ by {dp.max()}"


def check_camera_soft(c, frame, draws, mats, ref, ibl, consts, pcss):
    """What test_canvas_rt_pbr.check_camera_pbr checks but the texel read-back, through rt_render_pbr_soft."""
    _set(c, ibl, consts, pcss)
    c.rt_render_pbr_soft(frame, draws, mats)
    color, depth, vel = c.rt_resolve()
    pq, ids = c.rt_resolve_prequant(), c.rt_resolve_ids()
    compare_planes(color, depth, vel, pq, ids, ref, f"pbr-soft frame {frame.width}x{frame.height}")
    assert c.rt_stats() == ref["counters"]
    return color, depth, vel


def check_soft(c, view, lvp, draws, mats, w=W, h=H, sm=SM, tile=(80, 80), ibl=IBL, consts=None, pcss=None, casters_from=0, **kw):
    """Both passes against the restatements -> ((color, depth, velocity), the reference's planes)."""
    ref_sm = R.ref_shadow(sm, lvp, draws[casters_from:], tile)
    c.rt_render_shadow(sm, lvp, draws[casters_from:], ref_tile=tile)
    bad = np.argwhere(_bits(c.rt_resolve_shadow()) != _bits(ref_sm))
    assert bad.size == 0, f"{len(bad)} shadow-map texels differ, first {bad[:4].tolist()}"
    frame = Q.pbr_soft_frame(view, lvp, w, h, tile, **kw)
    ref = Q.ref_render_pbr_soft(frame, draws, mats, ref_sm if frame.use_shadow else None, ibl, consts, pcss)
    try:
        got = check_camera_soft(c, frame, draws, mats, ref, ibl, consts, pcss)
    finally:
        _set(c, None, None, None)
    return got, ref


def _pcss(key):
    return None if Q.GPU_PCSS[key] is None else S.demo_pcss(**Q.GPU_PCSS[key])


@pytest.mark.parametrize("tile", [(160, 160), (80, 80), (64, 48)], ids=["tile160", "tile80", "tile64x48"])
@pytest.mark.parametrize("use_shadow", [True, False], ids=["map", "no-map"])
def test_demo_in_miniature(ctx, use_shadow, tile):
    """160 x 120 over a 96^2 map, the demo's constants: the 18-texel search reaches the map's border."""
    view, lvp, draws, mats = P.demo_scene()
    (_, _, vel), ref = check_soft(ctx, view, lvp, draws, mats, tile=tile, use_shadow=use_shadow)
    assert vel.any()                                   # this demo has a motion buffer
    fac = ref["prequant"][..., 3][ref["tri_id"] >= 0]
    assert (fac == 1.0).all() if not use_shadow else ((fac > 0) & (fac < 1)).sum() > 3000


def test_pcf_flag_has_no_effect(ctx):
    view, lvp, draws, mats = P.demo_scene()
    (a, _, _), _ = check_soft(ctx, view, lvp, draws, mats, pcf=True)
    (b, _, _), _ = check_soft(ctx, view, lvp, draws, mats, pcf=False)
    assert np.array_equal(a, b)


@pytest.mark.parametrize("which", ["rough", "metal"])
@pytest.mark.parametrize("name", Q.EDGE_NAMES)
def test_scene(ctx, name, which):
    """test_canvas_rt_ref's edge scenes under the two edge-case materials: near-plane clipping and both windings feed px,
    py and the velocity through the new path; 'outside' has receivers outside the light's box."""
    view, lvp, draws, mats = P.edge_scene(name, which)
    check_soft(ctx, view, lvp, draws, mats)


def test_floor_left_out_of_the_shadow_pass(ctx):
    """Empty centre texels under the floor's fragments, taps on empty texels around the objects' shadows."""
    view, lvp, draws, mats = P.demo_scene()
    check_soft(ctx, view, lvp, draws, mats, casters_from=1)


@pytest.mark.parametrize("size,sm", [((1, 1), 8), ((33, 9), 50), ((31, 7), 50), ((160, 120), (96, 40)), ((160, 120), (1, 1))],
                         ids=["1x1", "33x9", "31x7", "map96x40", "map1x1"])
def test_frame_and_map_sizes(ctx, size, sm):
    """One pixel either side of the 32 x 8 tile; a non-square map (under the widened constants) and a one-texel map."""
    w, h = size
    view, proj = R.camera(w, h)
    _, lvp, draws, mats = P.demo_scene()
    draws = [R._rt_draw(d.mesh, d.model, view, proj, color=d.base_color, tex=d.albedo_tex) for d in draws]
    check_soft(ctx, view, lvp, draws, mats, w=w, h=h, sm=sm, pcss=_pcss("wide") if sm == (96, 40) else None)


@pytest.mark.parametrize("key", ["wide", "no-blockers", "no-taps", "wrap", "wide-light"])
def test_other_pcss_constants(ctx, key):
    view, lvp, draws, mats = P.demo_scene()
    _, ref = check_soft(ctx, view, lvp, draws, mats, pcss=_pcss(key))
    if key in ("no-blockers", "no-taps"):
        assert (ref["prequant"][..., 3][ref["tri_id"] >= 0] == 1.0).all()


@pytest.mark.parametrize("consts", [dict(exposure=0.9, min_roughness=0.1, direct_intensity=5.0), P.SATURATING], ids=["other", "saturating"])
def test_other_pbr_constants(ctx, consts):
    view, lvp, draws, mats = P.demo_scene()
    (color, _, _), _ = check_soft(ctx, view, lvp, draws, mats, consts=P.demo_consts(**consts))
    if consts is P.SATURATING:
        assert (color[..., :3] == 255).sum() > 1000


def test_without_an_ibl_and_with_one_replaced(ctx):
    """No IBL: where the light does not reach, the colour is exactly 0 (no minimum ambient).  Then an IBL of other sizes
    set after a frame with the first: the second frame uses the new levels."""
    view, lvp, draws, mats = P.demo_scene()
    (color, _, _), ref = check_soft(ctx, view, lvp, draws, mats, ibl=None)
    assert ((color[..., :3] == 0).all(-1) & (ref["tri_id"] >= 0)).sum() > 100
    other = P.make_ibl(3, 5, 6, 3)                      # irradiance 5^2, specular 6, 3, 1
    (first, _, _), _ = check_soft(ctx, view, lvp, draws, mats, ibl=IBL)
    (second, _, _), _ = check_soft(ctx, view, lvp, draws, mats, ibl=other)
    assert (first != second).any() and (first != color).any()


def test_texel_identity(ctx):
    """test_canvas_rt_pbr_soft_ref.texel_frame under the same bar; from the restatement alone, a neighbouring texel would
    move a channel of at least 95 % of the textured pixels by more than ten times that bar."""
    frame, draws, mats, ibl, consts, ref = Q.texel_frame()
    least = Q.texel_sensitivity()
    share = float((least > 10 * helpers.TOL * 255.0).mean())
    print(f"{len(least)} textured pixels, {100 * share:.2f} % pinned (smallest move {least.min():.3g})")
    assert share >= 0.95
    try:
        check_camera_soft(ctx, frame, draws, mats, ref, ibl, consts, None)
    finally:
        _set(ctx, None, None, None)


def test_frame_size_sequence_alternating_shadings(ctx):
    """One context through shadings 3, 1, 3, 0, 3, 2, 1, 3 over two alternating frame sizes (after 1 x 1): the rotation
    table of one size is built for shading 1 and reused by 3, rebuilt for 3 and reused by 1, and the frames of the other
    shadings still equal their own references."""
    steps = [((1, 1), 8, 3), ((33, 31), 50, 1), ((160, 120), 96, 3), ((33, 31), 50, 0), ((33, 31), 8, 3), ((160, 120), 96, 2),
             ((160, 120), 96, 1), ((33, 31), 50, 3)]
    for (w, h), sm, shading in steps:
        view, proj = R.camera(w, h)
        _, lvp, draws, mats = P.demo_scene()
        draws = [R._rt_draw(d.mesh, d.model, view, proj, color=d.base_color, tex=d.albedo_tex) for d in draws]
        if shading == 3:
            check_soft(ctx, view, lvp, draws, mats, w=w, h=h, sm=sm)
        elif shading == 2:
            ref_sm = R.ref_shadow(sm, lvp, draws)
            ctx.rt_render_shadow(sm, lvp, draws)
            frame = P.pbr_frame(view, lvp, w, h)
            ref = P.ref_render_pbr(frame, draws, mats, ref_sm, IBL)
            ctx.rt_set_ibl(*IBL)
            try:
                ctx.rt_render_pbr(frame, draws, mats)
                color, depth, vel = ctx.rt_resolve()
                compare_planes(color, depth, vel, ctx.rt_resolve_prequant(), ctx.rt_resolve_ids(), ref, f"shading 2 {w}x{h}")
            finally:
                ctx.rt_set_ibl(None)
        elif shading == 1:
            ref_sm = R.ref_shadow(sm, lvp, draws)
            ctx.rt_render_shadow(sm, lvp, draws)
            frame = S.soft_frame(view, lvp, w, h)
            T.check_camera(ctx, frame, draws, S.ref_render_soft(frame, draws, ref_sm))
        else:
            T.check_both(ctx, view, lvp, draws, w=w, h=h, sm=sm)


def test_rejections():
    import shs_gpu
    view, lvp, draws, mats = P.edge_scene("windings", "rough")
    with shs_gpu.Context(0) as c:
        frame = Q.pbr_soft_frame(view, lvp)

        def rejected(call, what):
            with pytest.raises(shs_gpu.ShsError) as e:
                call()
            assert e.value.code == -1, what

        rejected(lambda: c.rt_render_pbr_soft(frame, draws, mats), "SHS_RT_USE_SHADOW before any shadow pass")
        c.rt_render_shadow(SM, lvp, draws)
        for shading in (0, 1, 2, -1, 4):
            rejected(lambda: c.rt_render_pbr_soft(dataclasses.replace(frame, shading=shading), draws, mats), f"shading {shading}")
        rejected(lambda: c.rt_render_pbr_soft(frame, draws, mats[:-1]), "fewer materials than draws")
        rejected(lambda: c.rt_render_pbr_soft(frame, draws, mats + mats[:1]), "more materials than draws")
        rejected(lambda: c.rt_render_pbr_soft(frame, [dataclasses.replace(draws[0], mesh=999)] + draws[1:], mats), "unknown mesh")
        rejected(lambda: c.rt_render_pbr_soft(frame, [dataclasses.replace(draws[0], albedo_tex=77)] + draws[1:], mats), "unknown texture")
        rejected(lambda: c.rt_render_pbr_soft(dataclasses.replace(frame, width=0), draws, mats), "width 0")
        for call in (lambda: c.rt_render(frame, draws), lambda: c.rt_render_pbr(frame, draws, mats)):   # neither takes shading 3
            with pytest.raises(shs_gpu.ShsError) as e:
                call()
            assert e.value.code == -1 and "shading" in str(e.value)
        # the context still renders a correct shading-3 frame
        ref_sm = R.ref_shadow(SM, lvp, draws)
        ref = Q.ref_render_pbr_soft(frame, draws, mats, ref_sm, IBL)
        c.rt_set_ibl(*IBL)
        c.rt_render_pbr_soft(frame, draws, mats)
        color, depth, vel = c.rt_resolve()
        compare_planes(color, depth, vel, c.rt_resolve_prequant(), c.rt_resolve_ids(), ref, "after the rejections")
        assert (c.rt_resolve_ids() >= 0).sum() > 1000


def test_the_demos_whole_frame_on_the_device(ctx, oracle_mod):
    """hello_pbr_light_shafts.cpp's frame at 160 x 120 with 8 shaft steps, enqueued without a resolve in between: PASS0, the
    analytic sky and shading 3, shs_canvas_light_shafts over shs_rt_device_targets and shs_rt_device_shadow_map,
    shs_canvas_motion_blur over its output.  Each stage against its restatement run on the device's own output of the stage
    before it, so that a byte the parity rule allows does not travel."""
    import torch
    from shs_gpu import _abi
    _P = ctypes.c_void_p
    view, lvp, draws, mats = P.demo_scene()
    _, proj = R.camera()
    tile = (160, 160)
    sky = Q.chain_sky()
    frame = Q.pbr_soft_frame(view, lvp, tile=tile)
    ctx._on_torch_stream()
    out = torch.empty((H, W, 4), dtype=torch.uint8, device="cuda")
    out_pq = torch.empty((H, W, 4), dtype=torch.float32, device="cuda")
    dst = torch.empty((H, W, 4), dtype=torch.uint8, device="cuda")
    _set(ctx, IBL, None, None)
    ctx.rt_set_sky(sky)
    try:
        ctx.rt_render_shadow(SM, lvp, draws, ref_tile=tile)
        ctx.rt_render_pbr_soft(frame, draws, mats)
        c_dev, d_dev, v_dev = ctx.rt_device_targets()
        m_dev, m_size = ctx.rt_device_shadow_map()
        blank = np.zeros((H, W), F)
        sd = L.make_desc(Q.shafts_inputs(np.zeros((H, W, 4), np.uint8), blank, np.zeros((m_size[1], m_size[0]), F), lvp), Q.SHAFT_PARAMS)
        ctx._check(ctx._lib.shs_canvas_light_shafts(ctx._h, ctypes.byref(sd), _P(c_dev), _P(d_dev), _P(m_dev), _P(out.data_ptr()),
                                                    _P(out_pq.data_ptr()), ctx.CANVAS_DEVICE))
        md = _abi.CanvasMotionBlurDescC()
        md.width, md.height = W, H
        for k in range(16):
            md.curr_view[k] = md.prev_view[k] = float(view[k])
            md.curr_proj[k] = md.prev_proj[k] = float(proj[k])
        md.samples, md.strength, md.w_obj, md.w_cam, md.soft_knee, md.knee_px, md.max_px = 12, 0.85, 1.0, 0.35, 1, 18.0, 22.0
        ctx._check(ctx._lib.shs_canvas_motion_blur(ctx._h, ctypes.byref(md), _P(out.data_ptr()), _P(d_dev), _P(v_dev), _P(dst.data_ptr()),
                                                   ctx.CANVAS_DEVICE))
        ctx.synchronize()
        shadow = ctx.rt_resolve_shadow()
        color, depth, vel = ctx.rt_resolve()
        pq, ids = ctx.rt_resolve_prequant(), ctx.rt_resolve_ids()
    finally:
        ctx.rt_set_sky(None)
        _set(ctx, None, None, None)
    shafts, shafts_pq, blurred = out.cpu().numpy(), out_pq.cpu().numpy(), dst.cpu().numpy()
    # PASS0
    ref_sm = R.ref_shadow(SM, lvp, draws, tile)
    assert np.array_equal(_bits(shadow), _bits(ref_sm))
    # the sky and PASS1
    ref = K.ref_compose(sky, Q.ref_render_pbr_soft(frame, draws, mats, ref_sm, IBL))
    compare_planes(color, depth, vel, pq, ids, ref, "whole frame, PASS1 over the sky")
    assert (ids < 0).sum() > 3000 and (color[ids < 0] != np.array(frame.clear_color, np.uint8)).any(-1).mean() > 0.99
    # PASS1.5 over the device's colour, depth and map
    inp = Q.shafts_inputs(color, depth, shadow, lvp)
    want = L.ref_pass(inp, Q.SHAFT_PARAMS)
    assert L.marched(want["pq"]).sum() > 2000
    LS._check(shafts, shafts_pq, inp, want, "whole frame, light shafts")
    assert (shafts != color).any()
    # PASS2 over the device's shafts output
    want = oracle_mod.canvas_motion_blur(shafts, depth, vel, view, proj, view, proj)
    bad = np.argwhere((blurred != want).any(-1))
    assert bad.size == 0, f"{len(bad)} blurred pixels differ, first {bad[:4].tolist()}"
    assert (blurred != shafts).any()
