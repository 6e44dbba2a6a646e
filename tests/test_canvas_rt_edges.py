"""The Canvas render-target raster on the GPU at its own documented special cases, against tests/canvas_rt_ref:
test_canvas_rt_edges_ref.py holds the scenes, says for each which lines of the reference state the rule, and shows on
the CPU that the restatement's frame has the phenomenon in it.

Everything is compared as test_canvas_rt.check_both / check_camera compare it -- shadow map, view-z depth, velocity and
shadow factor bit-exact, ids, texel indices and counters equal, colours through helpers.assert_color_parity, on every
pixel -- and the other shadings through their own files' checkers.  The one exception is the scene whose normals and
UVs are not finite, where the planes hold NaNs: see test_nonfinite_attributes."""
import dataclasses

import numpy as np
import pytest

import helpers
import test_canvas_rt as T
import test_canvas_rt_edges_ref as E
import test_canvas_rt_pbr as TP
import test_canvas_rt_pbr_soft as TQ
import test_canvas_rt_ref as R
import test_canvas_rt_sky as TK
import test_canvas_rt_sky_ref as K
import test_canvas_rt_soft as TS
from test_canvas_rt_ref import F

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import shs_gpu
    c = shs_gpu.Context(0)
    yield c
    c.close()


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def check(c, scene):
    view, lvp, draws, opts = scene
    return T.check_both(c, view, lvp, draws, **opts)


@pytest.mark.parametrize("tile", E.JOBS, ids=[f"{t[0]}x{t[1]}" for t in E.JOBS])
def test_small_jobs(ctx, tile):
    """Reference tile jobs from one pixel to beyond the frame over 400 slivers: several jobs per 32 x 8 raster tile, a
    job's corner pixel in every tile."""
    check(ctx, E.scene_small_jobs(tile))


@pytest.mark.parametrize("tile", [(7, 5), (33, 9)], ids=["7x5", "33x9"])
def test_demo_through_small_jobs(ctx, tile):
    check(ctx, E.scene_demo_small_jobs(tile))


def test_no_colour(ctx):
    """A fragment with invw_sum <= 1e-8 keeps its depth and leaves the pixel's colour, velocity and id alone."""
    (_, depth, _), ref = check(ctx, E.scene_no_colour())
    ids = ctx.rt_resolve_ids()
    assert ((np.abs(depth - F(0.3)) < 1e-6) & (ids == -1)).sum() > 100 and not (ids == 2).any()


@pytest.mark.parametrize("kind", E.RB_KINDS)
@pytest.mark.parametrize("n_tris", E.RB_SIZES)
def test_round_boundaries(ctx, n_tris, kind):
    """Ties and nearer / farther pairs on either side of a 256-record round, in submissions of exactly 256, 258, 512 and
    516 camera records (the last: 258 shadow-pass records)."""
    check(ctx, E.scene_round_boundaries(n_tris, kind))


def test_nonfinite_positions(ctx):
    (_, depth, vel), ref = check(ctx, E.scene_nonfinite())
    assert ref["counters"] == E.NF_COUNTERS
    assert np.isfinite(depth).all() and np.isfinite(vel).all() and np.isfinite(ctx.rt_resolve_prequant()).all()


def test_nonfinite_attributes(ctx):
    """NaN and infinite normals and UVs on shown, textured triangles: the planes hold NaNs, which no tolerance compares.
    The NaN masks of the pre-truncation floats are equal; where the reference's are NaN the colour bytes are equal (the
    truncation of a NaN is 0); everywhere else the usual rule holds on the planes with the NaNs zeroed on both sides --
    the same tolerance, no pixel excused; depth, velocity, shadow factor, ids, the texel of every finite pixel and the
    counters as ever."""
    view, lvp, draws, opts = E.scene_nonfinite_attributes()
    sm = opts["sm"]
    ref_sm = R.ref_shadow(sm, lvp, draws)
    ctx.rt_render_shadow(sm, lvp, draws)
    assert np.array_equal(_bits(ctx.rt_resolve_shadow()), _bits(ref_sm))
    frame = R._frame(view, lvp, opts["w"], opts["h"])
    ref = R.ref_render(frame, draws, ref_sm)
    ctx.rt_render(frame, draws)
    color, depth, vel = ctx.rt_resolve()
    pq, ids = ctx.rt_resolve_prequant(), ctx.rt_resolve_ids()
    helpers.assert_depth_bitexact(depth, ref["depth"])
    assert np.array_equal(ids, ref["tri_id"])
    assert np.array_equal(_bits(vel), _bits(ref["velocity"]))
    nan_g, nan_r = np.isnan(pq), np.isnan(ref["prequant"])
    bad = np.argwhere(nan_g != nan_r)
    assert bad.size == 0, f"{len(bad)} NaN flags differ, first {bad[:4].tolist()}"
    assert nan_r[..., :3].any() and not nan_r[..., 3].any()
    px_nan = nan_r.any(-1)
    assert np.array_equal(color[px_nan], ref["color"][px_nan])
    assert np.array_equal(_bits(pq[..., 3]), _bits(ref["prequant"][..., 3]))
    g0, r0 = np.where(nan_g, F(0), pq), np.where(nan_r, F(0), ref["prequant"])
    helpers.assert_color_parity(color, ref["color"], g0, r0)
    assert np.abs(g0[..., :3] - r0[..., :3]).max() <= helpers.TOL * 255.0
    fin = (ids >= 0) & ~px_nan
    idx = R.texel_of_prequant(draws[0].albedo_tex, np.where(fin[..., None], pq, F(0)))
    wrong = fin & (idx != ref["texel"])
    assert fin.sum() > 200 and not wrong.any(), f"{int(wrong.sum())} pixels sampled another texel"
    assert ctx.rt_stats() == ref["counters"]


def test_giant(ctx):
    check(ctx, E.scene_giant())


def test_thresholds(ctx):
    check(ctx, E.scene_thresholds())


@pytest.mark.parametrize("pcf", [True, False], ids=["pcf", "compare"])
def test_perspective_light(ctx, pcf):
    """A light matrix whose w is not 1: the cx / cw of the shadow setup and of the camera pass's lookup, casters across
    the light's w = 0 plane."""
    check(ctx, E.scene_perspective_light(pcf))


# ---- the other instantiations of the raster kernel --------------------------------------------------------------------

@pytest.mark.parametrize("name", E.SHADING_NAMES)
def test_scene_soft(ctx, name):
    """Shading 1 (test_canvas_rt_soft.check_soft)."""
    view, lvp, draws, opts = E.shading_scene(name)
    TS.check_soft(ctx, view, lvp, draws, **opts)


@pytest.mark.parametrize("which", ["rough", "metal"])
@pytest.mark.parametrize("name", E.SHADING_NAMES)
def test_scene_pbr(ctx, name, which):
    """Shading 2 (test_canvas_rt_pbr.check_pbr)."""
    view, lvp, draws, opts = E.shading_scene(name)
    TP.check_pbr(ctx, view, lvp, draws, E.edge_materials(draws, which), **opts)


@pytest.mark.parametrize("which", ["rough", "metal"])
@pytest.mark.parametrize("name", E.SHADING_NAMES)
def test_scene_pbr_soft(ctx, name, which):
    """Shading 3 (test_canvas_rt_pbr_soft.check_soft)."""
    view, lvp, draws, opts = E.shading_scene(name)
    TQ.check_soft(ctx, view, lvp, draws, E.edge_materials(draws, which), **opts)


def test_no_colour_under_a_sky(ctx):
    """The reference draws the sky first: the pixels that hold the near depth and no fragment show sky."""
    view, lvp, draws, opts = E.scene_no_colour()
    w, h, sm = opts["w"], opts["h"], opts["sm"]
    sky = K.analytic_sky(K.elevated(5.0), K.REINHARD, fov_degrees=60.0, **K.camera_vectors((0.0, 0.2, 1.0)))
    ref_sm = R.ref_shadow(sm, lvp, draws)
    frame = R._frame(view, lvp, w, h)
    plain = R.ref_render(frame, draws, ref_sm)
    ref = K.ref_compose(sky, plain)
    ctx.rt_render_shadow(sm, lvp, draws)
    ctx.rt_set_sky(sky)
    try:
        ctx.rt_render(frame, draws)
        got = TK._planes(ctx)
    finally:
        ctx.rt_set_sky(None)
    TK.check_frame(got, ref)
    bare = (np.abs(got["depth"] - F(0.3)) < 1e-6) & (got["tri_id"] == -1)
    assert bare.sum() > 100 and (got["color"][bare] != np.array(frame.clear_color, np.uint8)).any(-1).all()
    assert ctx.rt_stats() == plain["counters"]


def test_sequence(ctx):
    """Frame size, map size, job size and record count change from frame to frame through one context."""
    for scene in (E.scene_small_jobs((1, 1)), E.scene_giant(), E.scene_round_boundaries(258, "tie"),
                  E.scene_round_boundaries(129, "far_first"), E.scene_small_jobs((33, 9))):
        check(ctx, scene)
