"""The PCSS soft-shadow camera pass on the GPU (shs_rt_render with shading = 1, shs_rt_set_pcss, shs_rt_pcss_samples)
against tests/canvas_rt_soft_ref (test_canvas_rt_soft_ref.py holds the wrapper, the sample sets and what pins the
reference on the CPU; the scenes and the camera are test_canvas_rt_ref's).

Per frame, on every pixel, none excused (test_canvas_rt.check_camera): the view-z depth, the velocity (all zero) and
the shadow factor (the prequant plane's alpha) bit-exact; the shading sub-triangle equal; the texel index of every
textured pixel equal; colours through helpers.assert_color_parity with the pre-truncation floats within
helpers.TOL * 255; the setup counters equal.  PASS0 is the hard demo's and is compared as there."""
import dataclasses

import numpy as np
import pytest

import test_canvas_rt as T
import test_canvas_rt_ref as R
import test_canvas_rt_soft_ref as S
from test_canvas_rt_ref import F, H, SM, W

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import shs_gpu
    c = shs_gpu.Context(0)
    yield c
    c.close()


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def check_soft(c, view, lvp, draws, w=W, h=H, sm=SM, tile=(80, 80), pcss=None, casters_from=0, **kw):
    """Both passes against the restatements; pcss: keyword changes to the demo's constants."""
    k = S.demo_pcss(**(pcss or {}))
    casters = draws[casters_from:]
    ref_sm = R.ref_shadow(sm, lvp, casters, tile)
    c.rt_render_shadow(sm, lvp, casters, ref_tile=tile)
    bad = np.argwhere(_bits(c.rt_resolve_shadow()) != _bits(ref_sm))
    assert bad.size == 0, f"{len(bad)} shadow-map texels differ, first {bad[:4].tolist()}"
    frame = S.soft_frame(view, lvp, w, h, tile, **kw)
    ref = S.ref_render_soft(frame, draws, ref_sm if frame.use_shadow else None, k)
    assert not ref["velocity"].any()
    c.rt_set_pcss(k)
    try:
        got = T.check_camera(c, frame, draws, ref)
    finally:
        c.rt_set_pcss(None)
    return got, ref


@pytest.mark.parametrize("tile", [(80, 80), (160, 160), (64, 48)], ids=["tile80", "tile160", "tile64x48"])
@pytest.mark.parametrize("pcss", [None, S.WIDE], ids=["demo", "wide"])
def test_demo_in_miniature(ctx, pcss, tile):
    """160 x 120 over a 96^2 map.  With the demo's constants every radius sits at the min clamp; the widened set makes
    it span both clamps (test_canvas_rt_soft_ref.NEED lists what the reference shows)."""
    view, lvp, draws = R.scene_demo()
    check_soft(ctx, view, lvp, draws, tile=tile, pcss=pcss)


@pytest.mark.parametrize("casters_from", [0, 1], ids=["all-cast", "floor-does-not-cast"])
def test_demo_on_a_non_square_map(ctx, casters_from):
    view, lvp, draws = R.scene_demo()
    check_soft(ctx, view, lvp, draws, sm=(96, 50), pcss=S.WIDE, casters_from=casters_from)


def test_floor_left_out_of_the_shadow_pass(ctx):
    """Empty centre texels under most of the floor, PCF and blocker taps on empty texels around the shadows."""
    view, lvp, draws = R.scene_demo()
    check_soft(ctx, view, lvp, draws, pcss=S.WIDE, casters_from=1)


@pytest.mark.parametrize("pcss", [None, S.WIDE], ids=["demo", "wide"])
@pytest.mark.parametrize("name", ["windings", "near", "coincident", "outside"])
def test_scene(ctx, name, pcss):
    view, lvp, draws = R.SCENES[name]()
    check_soft(ctx, view, lvp, draws, pcss=pcss)


def test_without_a_shadow_map(ctx):
    view, lvp, draws = R.scene_demo()
    (_, _, vel), ref = check_soft(ctx, view, lvp, draws, use_shadow=False)
    assert not vel.any() and (ref["prequant"][..., 3][ref["tri_id"] >= 0] == 1.0).all()


def test_pcf_flag_has_no_effect(ctx):
    view, lvp, draws = R.scene_demo()
    planes = []
    for pcf in (True, False):
        (color, depth, vel), _ = check_soft(ctx, view, lvp, draws, pcss=S.WIDE, pcf=pcf)
        planes.append((color, depth, vel, ctx.rt_resolve_prequant(), ctx.rt_resolve_ids()))
    for a, b in zip(*planes):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))


def test_frame_size_sequence_alternating_shadings(ctx):
    """1x1, 33x31, 160x120 and 33x31 again through one context, shading 1, 0, 1, 0: the rotation table follows the
    size, and the hard frames still equal test_canvas_rt_ref's reference bit for bit."""
    for ((w, h), sm), shading in zip([((1, 1), 8), ((33, 31), 50), ((160, 120), 96), ((33, 31), 8)], (1, 0, 1, 0)):
        view, proj = R.camera(w, h)
        _, lvp, draws = R.scene_demo()
        draws = [R._rt_draw(d.mesh, d.model, view, proj, color=d.base_color, tex=d.albedo_tex) for d in draws]
        if shading:
            check_soft(ctx, view, lvp, draws, w=w, h=h, sm=sm, pcss=S.WIDE)
        else:
            T.check_both(ctx, view, lvp, draws, w=w, h=h, sm=sm)
    view, proj = R.camera(33, 31)                 # and a soft frame of a size seen before, after another size
    draws = [R._rt_draw(d.mesh, d.model, view, proj, color=d.base_color, tex=d.albedo_tex) for d in R.scene_demo()[2]]
    check_soft(ctx, view, R.scene_demo()[1], draws, w=33, h=31, sm=50, pcss=S.WIDE)


def test_samples_known_answers(ctx):
    for name, sm, k, uv, z, bias, pxpy, want, _ in S.known_cases():
        ctx.rt_set_pcss(k)
        got = ctx.rt_pcss_samples(sm, [uv], [z], [bias], [pxpy])
        ref = S.ref_pcss_samples(sm, [uv], [z], [bias], [pxpy], k)[0]
        assert _bits(got)[0] == _bits(ref)[0], (name, got[0], ref[0])
        if want is not None:
            assert got[0] == want, (name, got[0])
    ctx.rt_set_pcss(None)


@pytest.mark.parametrize("pcss", [None, S.WIDE, dict(blocker_samples=40, pcf_samples=33, light_uv_radius=0.02),
                                  dict(blocker_samples=64, pcf_samples=64, light_uv_radius=0.1)], ids=["demo", "wide", "wrap", "64"])
def test_samples_random(ctx, pcss):
    """4,096 random samples on a random 64 x 40 map with about a third of its texels empty: factors bit-exact."""
    k = S.demo_pcss(**(pcss or {}))
    sm, uv, z, bias, pxpy = S.random_samples()
    ctx.rt_set_pcss(k)
    try:
        got = ctx.rt_pcss_samples(sm, uv, z, bias, pxpy)
    finally:
        ctx.rt_set_pcss(None)
    ref = S.ref_pcss_samples(sm, uv, z, bias, pxpy, k)[0]
    bad = np.argwhere(_bits(got) != _bits(ref))
    assert bad.size == 0, f"{len(bad)} of {len(ref)} factors differ, first {bad[:4].ravel().tolist()}"
    assert ((ref > 0) & (ref < 1)).sum() > 500


def test_samples_count_wrap(ctx):
    """40 taps are the 32 offsets and the first 8 again, on the device as in the restatement."""
    sm, uv, z, bias, pxpy = S.wrap_samples()
    for nb, nt in ((40, 40), (40, 32), (40, 8)):
        k = S.demo_pcss(blocker_samples=nb, pcf_samples=nt, light_uv_radius=0.03)
        ctx.rt_set_pcss(k)
        got = ctx.rt_pcss_samples(sm, uv, z, bias, pxpy)
        assert np.array_equal(_bits(got), _bits(S.ref_pcss_samples(sm, uv, z, bias, pxpy, k)[0])), (nb, nt)
    ctx.rt_set_pcss(None)


def test_rejections():
    import shs_gpu
    view, lvp, draws = R.scene_windings()
    nan = float("nan")
    with shs_gpu.Context(0) as c:
        frame = S.soft_frame(view, lvp)
        with pytest.raises(shs_gpu.ShsError) as e:      # shading 1 with SHS_RT_USE_SHADOW before any shadow pass
            c.rt_render(frame, draws)
        assert e.value.code == -1
        c.rt_render_shadow(SM, lvp, draws)
        with pytest.raises(shs_gpu.ShsError) as e:
            c.rt_render(dataclasses.replace(frame, shading=2), draws)
        assert e.value.code == -1 and "shading" in str(e.value)
        with pytest.raises(shs_gpu.ShsError) as e:
            c.rt_render(dataclasses.replace(frame, shading=-1), draws)
        assert e.value.code == -1
        for bad in (dict(blocker_samples=65), dict(pcf_samples=65), dict(pcf_samples=-1), dict(epsilon=nan),
                    dict(light_uv_radius=float("inf")), dict(max_filter_texels=nan)):
            with pytest.raises(shs_gpu.ShsError) as e:
                c.rt_set_pcss(S.demo_pcss(**bad))
            assert e.value.code == -1, bad
        # the rejected constants were not kept, and the context still renders: the frame is the demo constants'
        ref_sm = R.ref_shadow(SM, lvp, draws)
        ref = S.ref_render_soft(frame, draws, ref_sm)
        T.check_camera(c, frame, draws, ref)
        assert (c.rt_resolve_ids() >= 0).sum() > 1000
