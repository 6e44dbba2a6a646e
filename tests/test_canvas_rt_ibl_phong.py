"""The two passes of hello_ibl_skybox_optimized.cpp / hello_ibl_skybox_xsimd.cpp on the GPU -- shs_rt_render_ibl_phong
(shs_rt_frame::shading 11) and shs_rt_render_shadow_edge -- against tests/canvas_rt_ibl_phong_ref
(test_canvas_rt_ibl_phong_ref.py holds the wrapper, the knob sets, the IBL, the scenes and what pins the reference on the CPU).

Shading 11, per frame, on every pixel of every plane, none excused (test_canvas_rt_skybox_ibl.compare_planes): the shading
sub-triangle, the view-z depth, the velocity and the shadow factor equal bit for bit; the pre-truncation colour floats within
helpers.TOL * 255; colour bytes equal but for a byte off by one where those floats agree within that bound
(helpers.assert_color_parity); the counters equal.  The reference's pow(., shininess) is the host's powf, the device's one
double-precision pow rounded once: test_shininess prints the largest difference for integer and for fractional exponents.
The IBL's every texel is a colour of its own (distinct_ibl).

The edge shadow pass: every texel bit for bit, for every scene, map size, tile job size and lane count."""
import ctypes
import dataclasses

import numpy as np
import pytest

import helpers
import test_canvas_rt_edges_ref as E
import test_canvas_rt_ibl_phong_ref as Q
import test_canvas_rt_ref as R
import test_canvas_rt_sky as TK
import test_canvas_rt_sky_ref as K
import test_canvas_rt_skybox_ibl_ref as I
from test_canvas_rt_pbr_soft_ref import EDGE_NAMES
from test_canvas_rt_ref import F, H, SM, W
from test_canvas_rt_skybox_ibl import _bits, compare_planes

pytestmark = pytest.mark.gpu
BAR = helpers.TOL * 255.0
TILE = (160, 160)


@pytest.fixture(scope="module")
def ctx():
    import shs_gpu
    c = shs_gpu.Context(0)
    yield c
    c.close()


def render_phong(c, ibl, sky, frame, draws, sets):
    c.rt_set_ibl(*((ibl[0], list(ibl[1])) if ibl is not None else (None,)))
    c.rt_set_sky(sky)
    try:
        c.rt_render_ibl_phong(frame, draws, sets)
        return TK._planes(c)
    finally:
        c.rt_set_sky(None)
        c.rt_set_ibl(None)


def check_phong(c, view, lvp, draws, sets=None, ibl="distinct", sky=None, w=W, h=H, sm=SM, tile=TILE, label="", **kw):
    """Both passes against the restatements -> (the device's planes, the reference's)."""
    sets = Q.knobs_for(draws) if sets is None else sets
    ibl = Q.distinct_ibl() if isinstance(ibl, str) else ibl
    ref_sm = R.ref_shadow(sm, lvp, draws, tile)
    c.rt_render_shadow(sm, lvp, draws, ref_tile=tile)
    bad = np.argwhere(_bits(c.rt_resolve_shadow()) != _bits(ref_sm))
    assert bad.size == 0, f"{len(bad)} shadow-map texels differ, first {bad[:4].tolist()}"
    frame = Q.phong_frame(view, lvp, w, h, tile, **kw)
    ref = Q.ref_render_phong(ibl, frame, draws, sets, ref_sm if frame.use_shadow else None, sky)
    got = render_phong(c, ibl, sky, frame, draws, sets)
    compare_planes(got, ref, label or f"shading 11, {w}x{h}")
    assert c.rt_stats() == ref["counters"]
    return got, ref


@pytest.mark.parametrize("tile", [(160, 160), (80, 80), (64, 48)], ids=["tile160", "tile80", "tile64x48"])
@pytest.mark.parametrize("use_shadow,pcf", [(True, True), (True, False), (False, True)], ids=["pcf", "compare", "no-map"])
@pytest.mark.parametrize("bound", [True, False], ids=["ibl", "no-ibl"])
def test_demo_in_miniature(ctx, bound, use_shadow, pcf, tile):
    """The floor, the monkey (untextured) and the textured quad with the demo's three knob sets, 160 x 120 over a 96^2 map."""
    view, lvp, draws = R.scene_demo()
    got, ref = check_phong(ctx, view, lvp, draws, ibl="distinct" if bound else None, tile=tile, use_shadow=use_shadow, pcf=pcf,
                           label=f"demo, ibl {bound}")
    shaded = ref["tri_id"] >= 0
    assert got["velocity"].any() and 3000 < shaded.sum() < W * H - 2000
    if bound:
        assert set(np.unique(ref["face_n"][shaded])) | set(np.unique(ref["face_r"][shaded])) >= set(range(6))
        assert len(np.unique(ref["lod"][shaded])) == 3                   # one lod per knob set
    else:
        assert (ref["face_n"] == -1).all()


def test_ibl_terms_are_there(ctx):
    """The frame with the IBL bound is not the frame without: the terms move most shaded pixels far beyond the bar."""
    view, lvp, draws = R.scene_demo()
    on, ref = check_phong(ctx, view, lvp, draws)
    off, _ = check_phong(ctx, view, lvp, draws, ibl=None)
    shaded = ref["tri_id"] >= 0
    assert (np.abs(on["prequant"][..., :3] - off["prequant"][..., :3]).max(-1)[shaded] > 100 * BAR).mean() > 0.9
    assert np.array_equal(_bits(on["prequant"][..., 3]), _bits(off["prequant"][..., 3]))


@pytest.mark.parametrize("size,sm", [((1, 1), 8), ((33, 9), 50), ((31, 7), 50)], ids=["1x1", "33x9", "31x7"])
def test_frame_sizes(ctx, size, sm):
    """One pixel either side of the 32 x 8 raster tile, and a single pixel; 2,082 records: more than one round of 256."""
    w, h = size
    view, proj = R.camera(w, h)
    _, lvp, draws = R.scene_demo()
    draws = [R._rt_draw(d.mesh, d.model, view, proj, color=d.base_color, tex=d.albedo_tex) for d in draws]
    check_phong(ctx, view, lvp, draws, w=w, h=h, sm=sm, label=f"{w}x{h}")


@pytest.mark.parametrize("name", EDGE_NAMES)
def test_scene(ctx, name):
    view, lvp, draws = R.SCENES[name]()
    check_phong(ctx, view, lvp, draws, tile=(80, 80), label=name)


@pytest.mark.parametrize("name", E.SHADING_NAMES)
def test_edge_scene(ctx, name):
    view, lvp, draws, opts = E.shading_scene(name)
    check_phong(ctx, view, lvp, draws, tile=(80, 80), label=name, **opts)


@pytest.mark.parametrize("shininess", Q.SHININESS)
def test_shininess(ctx, shininess):
    """Every draw at one exponent: integer-valued ones (0, 1, 32, 48, 96, 1000) and a fractional one (2.5).  The largest
    difference of a pre-truncation colour float from the restatement's is printed per exponent.  Measured on the MI355X
    (profiles/canvas_rt_ibl_phong.txt): 0 for each of the integer exponents, every float bit-identical; for 2.5 one float of
    57,600 off by one ulp, 1.53e-05, against the bar of 2.55e-03."""
    view, lvp, draws = R.scene_demo()
    sets = [dataclasses.replace(k, shininess=shininess) for k in Q.knobs_for(draws)]
    got, ref = check_phong(ctx, view, lvp, draws, sets=sets, label=f"shininess {shininess}")
    shaded = ref["tri_id"] >= 0
    d = np.abs(got["prequant"][..., :3] - ref["prequant"][..., :3])[shaded].max()
    kind = "integer" if float(shininess).is_integer() else "fractional"
    print(f"shininess {shininess} ({kind} exponent): largest colour-float difference {d:.3g} of a bar of {BAR:.3g}")
    if shininess == 0.0:
        assert (ref["spec"][shaded] == 1.0).all()
    else:
        assert len(np.unique(ref["spec"][shaded])) > 100


@pytest.mark.parametrize("which", ["cubemap", "none"])
def test_sky_behind_it(ctx, which):
    """The background pass follows shading 11 as every camera pass: the cubemap sky under the clamp encode, or the clear."""
    view, lvp, draws = R.scene_demo()
    got, ref = check_phong(ctx, view, lvp, draws, sky=I.demo_sky(which, K.CLAMP), label=f"sky {which}")
    empty = ref["tri_id"] < 0
    clear = np.array(Q.phong_frame(view, lvp).clear_color, np.uint8)
    if which == "none":
        assert (got["color"][empty] == clear).all()
    else:
        assert (got["color"][empty] != clear).any(-1).mean() > 0.99


def test_rejections():
    import shs_gpu
    import test_canvas_rt_pbr_ref as P
    nan, inf = float("nan"), float("inf")
    view, lvp, draws = R.scene_windings()
    sets = Q.knobs_for(draws)
    mats = [P.material(None) for _ in draws]
    ibl = Q.distinct_ibl()
    with shs_gpu.Context(0) as c:
        frame = Q.phong_frame(view, lvp, tile=(80, 80))
        ref_sm = R.ref_shadow(SM, lvp, draws)
        ref = Q.ref_render_phong(ibl, frame, draws, sets, ref_sm)

        def rejected(call, what):
            with pytest.raises(shs_gpu.ShsError) as e:
                call()
            assert e.value.code == -1, what

        def planes_are_still_there(what):
            compare_planes(TK._planes(c), ref, f"the planes after the rejection of {what}")

        rejected(lambda: c.rt_render_ibl_phong(frame, draws, sets), "SHS_RT_USE_SHADOW before any shadow pass")
        c.rt_render_shadow(SM, lvp, draws)
        compare_planes(render_phong(c, ibl, None, frame, draws, sets), ref, "the first frame")
        ik = I.knobs_for(draws)
        cases = [(f"shading {s}", lambda s=s: c.rt_render_ibl_phong(dataclasses.replace(frame, shading=s), draws, sets))
                 for s in (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 12, -1)]
        cases += [("shading 11 through shs_rt_render", lambda: c.rt_render(frame, draws)),
                  ("shading 11 through shs_rt_render_pbr", lambda: c.rt_render_pbr(frame, draws, mats)),
                  ("shading 11 through shs_rt_render_pbr_soft", lambda: c.rt_render_pbr_soft(frame, draws, mats)),
                  ("shading 11 through shs_rt_render_skybox_ibl", lambda: c.rt_render_skybox_ibl(frame, draws, ik)),
                  ("shading 11 through shs_rt_render_water",
                   lambda: c.rt_render_water(frame, draws, [shs_gpu.RtWaterDraw() for _ in draws], shs_gpu.RtWater())),
                  ("shading 11 through shs_rt_render_motion", lambda: c.rt_render_motion(frame, draws)),
                  ("shading 11 through shs_rt_render_plain", lambda: c.rt_render_plain(frame, draws)),
                  ("null ibl_draws", lambda: c.rt_render_ibl_phong(frame, draws, None))]
        cases += [(f"{name} = {bad}", lambda name=name, bad=bad: c.rt_render_ibl_phong(frame, draws, sets[:-1] + [dataclasses.replace(sets[-1], **{name: bad})]))
                  for name in ("ibl_ambient", "ibl_refl", "ibl_f0", "ibl_refl_mix", "shininess") for bad in (nan, inf, -inf)]
        cases += [("shininess = -1", lambda: c.rt_render_ibl_phong(frame, draws, [dataclasses.replace(sets[0], shininess=-1.0)] + sets[1:])),
                  ("shininess = -1e-30", lambda: c.rt_render_ibl_phong(frame, draws, [dataclasses.replace(sets[0], shininess=-1e-30)] + sets[1:])),
                  ("unknown mesh", lambda: c.rt_render_ibl_phong(frame, [dataclasses.replace(draws[0], mesh=999)] + draws[1:], sets)),
                  ("unknown texture", lambda: c.rt_render_ibl_phong(frame, [dataclasses.replace(draws[0], albedo_tex=77)] + draws[1:], sets)),
                  ("width 0", lambda: c.rt_render_ibl_phong(dataclasses.replace(frame, width=0), draws, sets))]
        for what, call in cases:
            rejected(call, what)
            planes_are_still_there(what)           # nothing was enqueued: the frame before is still in the planes
        # the edge shadow pass's rejections leave the map as it was
        before = c.rt_resolve_shadow()
        for lanes in (0, 3, 5, 32, -8):
            rejected(lambda lanes=lanes: c.rt_render_shadow_edge(SM, lvp, draws, lanes=lanes), f"lanes {lanes}")
        rejected(lambda: c.rt_render_shadow_edge(0, lvp, draws), "a map of size 0")
        rejected(lambda: c.rt_render_shadow_edge(SM, lvp, draws, ref_tile=(0, 8)), "a tile job of width 0")
        rejected(lambda: c.rt_render_shadow_edge(SM, lvp, [dataclasses.replace(draws[0], mesh=999)]), "an unknown mesh")
        assert np.array_equal(_bits(c.rt_resolve_shadow()), _bits(before))
        planes_are_still_there("the edge pass's rejections")
        with pytest.raises(shs_gpu.ShsError):                      # the Python wrapper's own count check
            c.rt_render_ibl_phong(frame, draws, sets[:-1])
        c.rt_render_ibl_phong(frame, [], None)                     # no draws and a null table is an empty frame
        assert (c.rt_resolve_ids() == -1).all()


# ---- the edge-function shadow pass ----------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(Q.EDGE_SCENES))
def test_shadow_edge(ctx, name):
    """Every scene of the CPU file over maps of 8^2, 50^2 and 96^2, tile jobs of (160, 160), (64, 48) and (7, 5) and 1, 4, 8 and
    16 lanes: every texel bit for bit."""
    lvp, casters = Q.EDGE_SCENES[name]()
    drawn = 0
    for size in Q.EDGE_MAPS:
        for tile in Q.EDGE_TILES:
            for lanes in Q.EDGE_LANES:
                ref = Q.ref_shadow_edge(size, lvp, casters, tile, lanes)
                ctx.rt_render_shadow_edge(size, lvp, casters, ref_tile=tile, lanes=lanes)
                got = ctx.rt_resolve_shadow()
                bad = np.argwhere(_bits(got) != _bits(ref))
                assert bad.size == 0, f"{name}, map {size}, tile {tile}, lanes {lanes}: {len(bad)} texels differ, first {bad[:4].tolist()}"
                drawn += int((ref < helpers.FLT_MAX).sum())
    if name != "left_of_map":
        assert drawn > 0


def test_lanes_give_three_maps_on_the_device(ctx):
    lvp, casters = Q.scene_thirds()
    maps = {}
    for lanes in (4, 8, 16):
        ctx.rt_render_shadow_edge(50, lvp, casters, lanes=lanes)
        maps[lanes] = ctx.rt_resolve_shadow()
    for a, b in ((4, 8), (8, 16), (4, 16)):
        assert (_bits(maps[a]) != _bits(maps[b])).any()


def test_camera_pass_reads_the_edge_map(ctx):
    """SHS_RT_USE_SHADOW after shs_rt_render_shadow_edge: shading 11 and shading 0 over the edge raster's map, which is not
    the barycentric raster's (back faces cast no shadow)."""
    view, lvp, draws = R.scene_demo()
    ref_sm = Q.ref_shadow_edge(SM, lvp, draws, TILE, 8)
    old_sm = R.ref_shadow(SM, lvp, draws, TILE)
    assert (_bits(ref_sm) != _bits(old_sm)).any()
    ctx.rt_render_shadow_edge(SM, lvp, draws, ref_tile=TILE, lanes=8)
    assert np.array_equal(_bits(ctx.rt_resolve_shadow()), _bits(ref_sm))
    dev, size = ctx.rt_device_shadow_map()
    assert dev and tuple(size) == (SM, SM)
    frame = Q.phong_frame(view, lvp)
    sets = Q.knobs_for(draws)
    ref = Q.ref_render_phong(Q.distinct_ibl(), frame, draws, sets, ref_sm)
    got = render_phong(ctx, Q.distinct_ibl(), None, frame, draws, sets)
    compare_planes(got, ref, "shading 11 over the edge map")
    assert len(np.unique(ref["prequant"][..., 3][ref["tri_id"] >= 0])) == 5
    hard = R._frame(view, lvp, tile=TILE)
    ctx.rt_render(hard, draws)
    import test_canvas_rt_pbr_soft as TQ
    color, depth, vel = ctx.rt_resolve()
    TQ.compare_planes(color, depth, vel, ctx.rt_resolve_prequant(), ctx.rt_resolve_ids(), R.ref_render(hard, draws, ref_sm), "shading 0 over the edge map")


# ---- the two whole frames ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("demo", ["optimized", "xsimd"])
def test_the_demos_whole_frame_on_the_device(ctx, oracle_mod, demo):
    """The frame of hello_ibl_skybox_optimized.cpp (PASS0: shs_rt_render_shadow) and of hello_ibl_skybox_xsimd.cpp (PASS0:
    shs_rt_render_shadow_edge, 8 lanes) at 160 x 120, enqueued without a resolve in between: tile jobs of 160, the cubemap
    sky under the clamp encode, shading 11, shs_canvas_motion_blur over shs_rt_device_targets with the demos' MB_* constants.
    The reference is chained from the restatements: the blur of the restatement's own planes, compared byte for byte."""
    import torch
    from shs_gpu import _abi
    _P = ctypes.c_void_p
    view, lvp, draws = R.scene_demo()
    _, proj = R.camera()
    sky = I.demo_sky("cubemap", K.CLAMP)
    ibl = Q.distinct_ibl()
    sets = Q.knobs_for(draws)
    frame = Q.phong_frame(view, lvp, tile=TILE)
    ctx._on_torch_stream()
    dst = torch.empty((H, W, 4), dtype=torch.uint8, device="cuda")
    ctx.rt_set_sky(sky)
    ctx.rt_set_ibl(ibl[0], list(ibl[1]))
    try:
        if demo == "xsimd":
            ctx.rt_render_shadow_edge(SM, lvp, draws, ref_tile=TILE, lanes=8)
        else:
            ctx.rt_render_shadow(SM, lvp, draws, ref_tile=TILE)
        ctx.rt_render_ibl_phong(frame, draws, sets)
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
        ctx.rt_set_ibl(None)
    blurred = dst.cpu().numpy()
    ref_sm = Q.ref_shadow_edge(SM, lvp, draws, TILE, 8) if demo == "xsimd" else R.ref_shadow(SM, lvp, draws, TILE)
    assert np.array_equal(_bits(shadow), _bits(ref_sm))
    ref = Q.ref_render_phong(ibl, frame, draws, sets, ref_sm, sky)
    compare_planes(got, ref, f"{demo}: PASS1 over the sky")
    ids = got["tri_id"]
    assert (ids < 0).sum() > 3000 and (got["color"][ids < 0] != np.array(frame.clear_color, np.uint8)).any(-1).mean() > 0.99
    want = oracle_mod.canvas_motion_blur(ref["color"], ref["depth"], ref["velocity"], view, proj, view, proj)
    bad = np.argwhere((blurred != want).any(-1))
    assert bad.size == 0, f"{demo}: {len(bad)} blurred pixels differ, first {bad[:4].tolist()}"
    assert (blurred != got["color"]).any()
