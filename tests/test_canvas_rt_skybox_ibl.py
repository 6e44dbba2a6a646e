"""The sky-lit camera pass on the GPU (shs_rt_render_skybox_ibl, shs_rt_frame::shading 4: PASS1 of hello_ibl_skybox.cpp)
against tests/canvas_rt_skybox_ibl_ref (test_canvas_rt_skybox_ibl_ref.py holds the wrapper, the knob sets, the skies and what
pins the reference on the CPU; the scenes are test_canvas_rt_ref's and test_canvas_rt_edges_ref's, the sky models
test_canvas_rt_sky_ref's).

Per frame, on every pixel of every plane, none excused (compare_planes): the shading sub-triangle, the view-z depth, the
velocity and the shadow factor (the prequant plane's fourth float) equal bit for bit; the pre-truncation colour floats
within helpers.TOL * 255 (a NaN where the reference has a NaN); colour bytes equal but for a byte off by one where those
floats agree within that bound (helpers.assert_color_parity).  The pixels no fragment shows are the background pass's and
go under the same rule.  The cubemap's every texel is a colour of its own (test_canvas_rt_skybox_ibl_ref.distinct_faces),
so another face, a flipped u or v or a neighbouring texel moves a channel by far more than that bound.
PASS0 is the hard demo's and is compared as there."""
import ctypes
import dataclasses

import numpy as np
import pytest

import helpers
import test_canvas_rt as T
import test_canvas_rt_edges_ref as E
import test_canvas_rt_pbr_ref as P
import test_canvas_rt_ref as R
import test_canvas_rt_sky as TK
import test_canvas_rt_sky_ref as K
import test_canvas_rt_skybox_ibl_ref as I
from test_canvas_rt_pbr_soft_ref import EDGE_NAMES
from test_canvas_rt_ref import F, H, SM, W

pytestmark = pytest.mark.gpu
BAR = helpers.TOL * 255.0


@pytest.fixture(scope="module")
def ctx():
    import shs_gpu
    c = shs_gpu.Context(0)
    yield c
    c.close()


def _bits(a):
    return P.canonical_bits(a)          # (every NaN is one NaN: the payload is not the reference's to pin)


def compare_planes(got, ref, label):
    bad = np.argwhere(got["tri_id"] != ref["tri_id"])
    assert bad.size == 0, f"{label}: {len(bad)} pixels shaded by another sub-triangle, first {bad[:4].tolist()}"
    bad = np.argwhere(_bits(got["depth"]) != _bits(ref["depth"]))
    assert bad.size == 0, f"{label}: {len(bad)} depths differ, first {bad[:4].tolist()}"
    bad = np.argwhere((_bits(got["velocity"]) != _bits(ref["velocity"])).any(-1))
    assert bad.size == 0, f"{label}: {len(bad)} velocities differ, first {bad[:4].tolist()}"
    pq, rq = got["prequant"], ref["prequant"]
    bad = np.argwhere(_bits(pq[..., 3]) != _bits(rq[..., 3]))
    assert bad.size == 0, f"{label}: {len(bad)} shadow factors differ, first {bad[:4].tolist()}"
    bad = np.argwhere(np.isnan(pq[..., :3]) != np.isnan(rq[..., :3]))
    assert bad.size == 0, f"{label}: {len(bad)} colour floats are NaN on one side only, first {bad[:4].tolist()}"
    with np.errstate(invalid="ignore"):
        dp = np.nan_to_num(np.abs(pq[..., :3] - rq[..., :3]), nan=0.0)
    n = helpers.assert_color_parity(got["color"], ref["color"], np.nan_to_num(pq), np.nan_to_num(rq))
    exact = int((_bits(pq[..., :3]) != _bits(rq[..., :3])).sum())
    worst = np.unravel_index(int(dp.argmax()), dp.shape)
    print(f"{label}: {exact} of {dp.size} colour floats not bit-identical, {n} bytes off by one, max float difference {dp.max():.3g} "
          f"(bar {BAR:.3g}) at {tuple(int(v) for v in worst)}: {pq[worst]!r} vs {rq[worst]!r}")
    assert dp.max() <= BAR, f"{label}: pre-truncation floats differ by {dp.max()}"


def render_ibl(c, sky, frame, draws, sets):
    c.rt_set_sky(sky)
    try:
        c.rt_render_skybox_ibl(frame, draws, sets)
        return TK._planes(c)
    finally:
        c.rt_set_sky(None)


def check_ibl(c, sky, view, lvp, draws, sets=None, w=W, h=H, sm=SM, tile=(160, 160), label="", **kw):
    """Both passes against the restatements -> (the device's planes, the reference's)."""
    sets = I.knobs_for(draws) if sets is None else sets
    ref_sm = R.ref_shadow(sm, lvp, draws, tile)
    c.rt_render_shadow(sm, lvp, draws, ref_tile=tile)
    bad = np.argwhere(_bits(c.rt_resolve_shadow()) != _bits(ref_sm))
    assert bad.size == 0, f"{len(bad)} shadow-map texels differ, first {bad[:4].tolist()}"
    frame = I.ibl_frame(view, lvp, w, h, tile, **kw)
    ref = I.ref_render_ibl(sky, frame, draws, sets, ref_sm if frame.use_shadow else None)
    got = render_ibl(c, sky, frame, draws, sets)
    compare_planes(got, ref, label or f"shading 4, {w}x{h}")
    assert c.rt_stats() == ref["counters"]
    return got, ref


@pytest.mark.parametrize("tile", [(160, 160), (80, 80), (64, 48)], ids=["tile160", "tile80", "tile64x48"])
@pytest.mark.parametrize("use_shadow,pcf", [(True, True), (True, False), (False, True)], ids=["pcf", "compare", "no-map"])
@pytest.mark.parametrize("which", I.SKY_NAMES)
def test_demo_in_miniature(ctx, which, use_shadow, pcf, tile):
    """The floor, the monkey (untextured) and the textured quad with the demo's three knob sets, 160 x 120 over a 96^2 map."""
    view, lvp, draws = R.scene_demo()
    got, ref = check_ibl(ctx, I.demo_sky(which), view, lvp, draws, tile=tile, use_shadow=use_shadow, pcf=pcf, label=f"demo under {which}")
    shaded = ref["tri_id"] >= 0
    assert got["velocity"].any() and 3000 < shaded.sum() < W * H - 2000
    clear = np.array(I.ibl_frame(view, lvp).clear_color, np.uint8)
    if which == "none":
        assert (got["color"][~shaded] == clear).all() and not got["prequant"][~shaded].any()
    else:
        assert (got["color"][~shaded] != clear).any(-1).mean() > 0.99
    if which == "cubemap":
        assert set(np.unique(ref["branch_n"][shaded])) | set(np.unique(ref["branch_r"][shaded])) >= set(range(6))


@pytest.mark.parametrize("size,sm", [((1, 1), 8), ((33, 9), 50), ((31, 7), 50)], ids=["1x1", "33x9", "31x7"])
def test_frame_sizes(ctx, size, sm):
    """One pixel either side of the 32 x 8 raster tile, and a single pixel.  The scene has 1,041 triangles, 2,082 records:
    every case stages more than one round of 256."""
    w, h = size
    view, proj = R.camera(w, h)
    _, lvp, draws = R.scene_demo()
    draws = [R._rt_draw(d.mesh, d.model, view, proj, color=d.base_color, tex=d.albedo_tex) for d in draws]
    assert 2 * sum(d.mesh.positions.shape[0] for d in draws) > 256
    for which in ("cubemap", "analytic"):
        check_ibl(ctx, I.demo_sky(which), view, lvp, draws, w=w, h=h, sm=sm, label=f"{w}x{h} under {which}")


@pytest.mark.parametrize("name", EDGE_NAMES)
def test_scene(ctx, name):
    """The raster's edge scenes under the cubemap sky: both windings, the near-plane set, coincident triangles, receivers
    outside the light's box."""
    view, lvp, draws = R.SCENES[name]()
    check_ibl(ctx, I.demo_sky("cubemap"), view, lvp, draws, tile=(80, 80), label=name)


@pytest.mark.parametrize("name", E.SHADING_NAMES)
def test_edge_scene(ctx, name):
    """test_canvas_rt_edges_ref's two scenes that run through every shading.  no_colour: a fragment with invw_sum <= 1e-8 keeps
    its depth and no colour; where nothing else is shown the background pass colours the pixel from the sky."""
    view, lvp, draws, opts = E.shading_scene(name)
    got, ref = check_ibl(ctx, I.demo_sky("cubemap"), view, lvp, draws, tile=(80, 80), label=name, **opts)
    if name == "no_colour":
        bare = (np.abs(got["depth"] - F(0.3)) < 1e-6) & (got["tri_id"] == -1)
        clear = np.array(I.ibl_frame(view, lvp).clear_color, np.uint8)
        assert bare.sum() > 100 and (got["color"][bare] != clear).any(-1).all() and (got["prequant"][bare][:, 3] == 1).all()


def _zero_normals(draws, which):
    d = draws[which]
    mesh = R.SoupMesh(d.mesh.positions, np.zeros_like(d.mesh.normals), getattr(d.mesh, "uvs", None))
    return [dataclasses.replace(d, mesh=mesh) if i == which else x for i, x in enumerate(draws)]


@pytest.mark.parametrize("which", ["cubemap", "analytic"])
def test_zero_length_normals(ctx, which):
    """The monkey's normals are zero: glm::normalize gives NaN, N is NaN in every fragment of the draw, and both sky models
    take their NaN paths (the cubemap: every texel out of bounds, NaN weights).  The colour floats are NaN where the
    reference's are and the bytes 0, as the x86-64 conversion of the reference gives."""
    view, lvp, draws = R.scene_demo()
    draws = _zero_normals(draws, 1)
    got, ref = check_ibl(ctx, I.demo_sky(which), view, lvp, draws, label=f"zero normals under {which}")
    who = T._draw_of(draws, ref["tri_id"])
    assert (who == 1).sum() > 500 and np.isnan(got["prequant"][who == 1][:, :3]).all() and (got["color"][who == 1][:, :3] == 0).all()
    assert not np.isnan(got["prequant"][who != 1]).any()


@pytest.mark.parametrize("key", list(I.EDGE_KNOBS))
def test_knobs_outside_0_1(ctx, key):
    view, lvp, draws = R.scene_demo()
    sets = I.EDGE_KNOBS[key]
    sky = I.demo_sky("cubemap")
    got, ref = check_ibl(ctx, sky, view, lvp, draws, sets=sets, label=f"knobs {key}")
    if key == "no-mix":
        # the reflection vanishes and the tint stays: the frame of ibl_refl = 0, and not the frame without a tint
        frame = I.ibl_frame(view, lvp)
        off = render_ibl(ctx, sky, frame, draws, [dataclasses.replace(k, ibl_refl=0.0, ibl_refl_mix=1.0) for k in sets])
        flat = render_ibl(ctx, sky, frame, draws, [dataclasses.replace(k, ibl_ambient=0.0) for k in sets])
        assert np.array_equal(_bits(off["prequant"]), _bits(got["prequant"])) and np.array_equal(off["color"], got["color"])
        shaded = ref["tri_id"] >= 0
        assert (np.abs(flat["prequant"][..., :3] - got["prequant"][..., :3]).max(-1)[shaded] > 100 * BAR).mean() > 0.9


@pytest.mark.parametrize("case", [c[0] for c in I.identity_cases()])
def test_white_base_is_shading_0s_frame_on_the_device(ctx, case):
    """White base colours, no texture, and either no sky or ibl_ambient = ibl_refl = 0: shs_rt_render (shading 0) and
    shs_rt_render_skybox_ibl on the same context give the same planes, bit for bit (the background pass, where a sky is
    bound, runs behind both)."""
    _, sky, sets = next(c for c in I.identity_cases() if c[0] == case)
    view, lvp, draws = R.scene_demo()
    draws = I._white(draws)
    ctx.rt_render_shadow(SM, lvp, draws)
    ctx.rt_set_sky(sky)
    try:
        ctx.rt_render(R._frame(view, lvp), draws)
        hard = TK._planes(ctx)
        ctx.rt_render_skybox_ibl(I.ibl_frame(view, lvp, tile=(80, 80)), draws, I.knobs_for(draws, sets))
        got = TK._planes(ctx)
    finally:
        ctx.rt_set_sky(None)
    for k in hard:
        assert np.array_equal(got[k].view(np.uint8), hard[k].view(np.uint8)), f"{case}: plane {k} differs"
    assert (hard["tri_id"] >= 0).sum() > 3000 and len(np.unique(hard["prequant"][..., 3])) == 5


def test_sequence_alternating_shadings_and_skies(ctx):
    """One context through shadings 0, 4, 2, 4, 0, 4 over two alternating frame sizes, the sky rebound between the shading-4
    frames (cubemap, then analytic, then none): each frame equals its own reference, so nothing of the frame, the sky or
    the knob table before it survives."""
    import test_canvas_rt_pbr_soft as TQ
    ibl = P.make_ibl()
    steps = [((33, 31), 50, 0, None), ((160, 120), 96, 4, "cubemap"), ((33, 31), 50, 2, None), ((160, 120), 96, 4, "analytic"),
             ((160, 120), 8, 0, None), ((33, 31), 50, 4, "none"), ((1, 1), 8, 4, "cubemap")]
    for (w, h), sm, shading, which in steps:
        view, proj = R.camera(w, h)
        _, lvp, draws, mats = P.demo_scene()
        draws = [R._rt_draw(d.mesh, d.model, view, proj, color=d.base_color, tex=d.albedo_tex) for d in draws]
        if shading == 4:
            sets = I.knobs_for(draws, I.EDGE_KNOBS["outside"] if which == "analytic" else None)
            check_ibl(ctx, I.demo_sky(which), view, lvp, draws, sets=sets, w=w, h=h, sm=sm, label=f"sequence: shading 4 under {which}")
        elif shading == 2:
            ref_sm = R.ref_shadow(sm, lvp, draws)
            ctx.rt_render_shadow(sm, lvp, draws)
            frame = P.pbr_frame(view, lvp, w, h)
            ref = P.ref_render_pbr(frame, draws, mats, ref_sm, ibl)
            ctx.rt_set_ibl(*ibl)
            try:
                ctx.rt_render_pbr(frame, draws, mats)
                color, depth, vel = ctx.rt_resolve()
                TQ.compare_planes(color, depth, vel, ctx.rt_resolve_prequant(), ctx.rt_resolve_ids(), ref, f"sequence: shading 2 {w}x{h}")
            finally:
                ctx.rt_set_ibl(None)
        else:
            T.check_both(ctx, view, lvp, draws, w=w, h=h, sm=sm)


def test_rejections():
    import shs_gpu
    nan, inf = float("nan"), float("inf")
    view, lvp, draws = R.scene_windings()
    sets = I.knobs_for(draws)
    mats = [P.material(None) for _ in draws]
    sky = I.demo_sky("cubemap")
    with shs_gpu.Context(0) as c:
        frame = I.ibl_frame(view, lvp, tile=(80, 80))
        ref_sm = R.ref_shadow(SM, lvp, draws)
        ref = I.ref_render_ibl(sky, frame, draws, sets, ref_sm)

        def rejected(call, what):
            with pytest.raises(shs_gpu.ShsError) as e:
                call()
            assert e.value.code == -1, what

        def still_right(what):
            compare_planes(render_ibl(c, sky, frame, draws, sets), ref, f"after the rejection of {what}")

        rejected(lambda: c.rt_render_skybox_ibl(frame, draws, sets), "SHS_RT_USE_SHADOW before any shadow pass")
        c.rt_render_shadow(SM, lvp, draws)
        still_right("SHS_RT_USE_SHADOW with no map")
        cases = [(f"shading {s}", lambda s=s: c.rt_render_skybox_ibl(dataclasses.replace(frame, shading=s), draws, sets)) for s in (0, 1, 2, 3, 5, -1)]
        cases += [("shading 4 through shs_rt_render", lambda: c.rt_render(frame, draws)),
                  ("shading 4 through shs_rt_render_pbr", lambda: c.rt_render_pbr(frame, draws, mats)),
                  ("shading 4 through shs_rt_render_pbr_soft", lambda: c.rt_render_pbr_soft(frame, draws, mats)),
                  ("null ibl_draws", lambda: c.rt_render_skybox_ibl(frame, draws, None))]
        cases += [(f"{name} = {bad}", lambda name=name, bad=bad: c.rt_render_skybox_ibl(frame, draws, sets[:-1] + [dataclasses.replace(sets[-1], **{name: bad})]))
                  for name in ("ibl_ambient", "ibl_refl", "ibl_f0", "ibl_refl_mix") for bad in (nan, inf, -inf)]
        cases += [("unknown mesh", lambda: c.rt_render_skybox_ibl(frame, [dataclasses.replace(draws[0], mesh=999)] + draws[1:], sets)),
                  ("unknown texture", lambda: c.rt_render_skybox_ibl(frame, [dataclasses.replace(draws[0], albedo_tex=77)] + draws[1:], sets)),
                  ("width 0", lambda: c.rt_render_skybox_ibl(dataclasses.replace(frame, width=0), draws, sets))]
        for what, call in cases:
            rejected(call, what)
            still_right(what)
        with pytest.raises(shs_gpu.ShsError):                      # the Python wrapper's own count check
            c.rt_render_skybox_ibl(frame, draws, sets[:-1])
        # no draws and a null table is a frame of sky
        c.rt_set_sky(sky)
        c.rt_render_skybox_ibl(frame, [], None)
        assert (c.rt_resolve_ids() == -1).all()
        c.rt_set_sky(None)


def test_the_demos_whole_frame_on_the_device(ctx, oracle_mod):
    """hello_ibl_skybox.cpp's frame at 160 x 120, enqueued without a resolve in between: PASS0 with tile jobs of 160, the
    cubemap sky under the clamp encode through the viewer's camera, shading 4, shs_canvas_motion_blur over
    shs_rt_device_targets (the demo's combined_motion_blur_pass :944-1060 is hello_pbr.cpp's :1128-1252 with the matrix
    inverse not hoisted and accessors instead of raw pointers: the same operations).  Each stage against its restatement, the
    blur on the device's own PASS1 output, so that a byte the parity rule allows does not travel."""
    import torch
    from shs_gpu import _abi
    _P = ctypes.c_void_p
    view, lvp, draws = R.scene_demo()
    _, proj = R.camera()
    tile = (160, 160)
    sky = I.demo_sky("cubemap", K.CLAMP)
    sets = I.knobs_for(draws)
    frame = I.ibl_frame(view, lvp, tile=tile)
    ctx._on_torch_stream()
    dst = torch.empty((H, W, 4), dtype=torch.uint8, device="cuda")
    ctx.rt_set_sky(sky)
    try:
        ctx.rt_render_shadow(SM, lvp, draws, ref_tile=tile)
        ctx.rt_render_skybox_ibl(frame, draws, sets)
        c_dev, d_dev, v_dev = ctx.rt_device_targets()
        md = _abi.CanvasMotionBlurDescC()
        md.width, md.height = W, H
        for k in range(16):
            md.curr_view[k] = md.prev_view[k] = float(view[k])
            md.curr_proj[k] = md.prev_proj[k] = float(proj[k])
        md.samples, md.strength, md.w_obj, md.w_cam, md.soft_knee, md.knee_px, md.max_px = 12, 0.85, 1.0, 0.35, 1, 18.0, 22.0
        ctx._check(ctx._lib.shs_canvas_motion_blur(ctx._h, ctypes.byref(md), _P(c_dev), _P(d_dev), _P(v_dev), _P(dst.data_ptr()),
                                                   ctx.CANVAS_DEVICE))
        ctx.synchronize()
        shadow = ctx.rt_resolve_shadow()
        got = TK._planes(ctx)
    finally:
        ctx.rt_set_sky(None)
    blurred = dst.cpu().numpy()
    # PASS0
    ref_sm = R.ref_shadow(SM, lvp, draws, tile)
    assert np.array_equal(_bits(shadow), _bits(ref_sm))
    # the sky and PASS1
    ref = I.ref_render_ibl(sky, frame, draws, sets, ref_sm)
    compare_planes(got, ref, "whole frame, PASS1 over the sky")
    ids = got["tri_id"]
    assert (ids < 0).sum() > 3000 and (got["color"][ids < 0] != np.array(frame.clear_color, np.uint8)).any(-1).mean() > 0.99
    # PASS2 over the device's colour
    want = oracle_mod.canvas_motion_blur(got["color"], got["depth"], got["velocity"], view, proj, view, proj)
    bad = np.argwhere((blurred != want).any(-1))
    assert bad.size == 0, f"{len(bad)} blurred pixels differ, first {bad[:4].tolist()}"
    assert (blurred != got["color"]).any()
