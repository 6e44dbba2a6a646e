"""The background of the Canvas render-target camera passes on the GPU (shs_rt_set_sky, shs_rt_sky_samples: the legacy
AnalyticSky / CubeMapSky behind shs_rt_render and shs_rt_render_pbr) against tests/canvas_rt_sky_ref
(test_canvas_rt_sky_ref.py holds the wrapper, the skies, the cameras, the sample sets and what pins the reference on the
CPU; the scenes are test_canvas_rt_ref's and test_canvas_rt_pbr_ref's).

The cubemap model is bit-exact.  The analytic model's three pows are products in double on the device and libm's powf in
the restatement, so its radiance is compared within helpers.TOL, absolute; cosGamma has no pow in it, so the branch a
sample takes -- disc, ring or neither -- must be the restatement's.  A frame's sky pixels go through
helpers.assert_color_parity with the pre-truncation floats within helpers.TOL * 255 (linear_to_srgb's pow is the
device's there and libm's here); the pixels that show a fragment equal the sky-less frame's bit for bit, in every plane."""
import dataclasses

import numpy as np
import pytest

import helpers
import test_canvas_rt_pbr_ref as P
import test_canvas_rt_ref as R
import test_canvas_rt_sky_ref as K
import test_canvas_rt_soft_ref as S
from test_canvas_rt_ref import F, H, SM, W

pytestmark = pytest.mark.gpu
IBL = P.make_ibl()
FRAME_SKIES = dict(K.frame_skies())
DEMO_SKIES = dict(K.demo_skies())


@pytest.fixture(scope="module")
def ctx():
    import shs_gpu
    c = shs_gpu.Context(0)
    yield c
    c.close()


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _planes(c):
    color, depth, vel = c.rt_resolve()
    return {"color": color, "depth": depth, "velocity": vel, "prequant": c.rt_resolve_prequant(), "tri_id": c.rt_resolve_ids()}


def _sample_set():
    return np.concatenate([K.random_directions(), np.array([e[1] for e in K.edge_directions()], F)])


# ---- shs_rt_sky_samples -------------------------------------------------------------------------------------

@pytest.mark.parametrize("faces,intensity", [(None, 1.0), (None, 3.0), ("odd", 0.37)], ids=["unit", "bright", "odd-sizes"])
def test_cubemap_samples_are_bit_exact(ctx, faces, intensity):
    """4,096 seeded directions plus the edge, zero-length, NaN and infinite ones over faces of 4x4, 5x3, 1x1, 7x2, 2x6 and 3x8
    texels: every float equal to the restatement's, a NaN where it has a NaN."""
    sky = K.cubemap_sky(K.make_faces(9, K.ODD_SIZES) if faces == "odd" else None, intensity)
    d = np.concatenate([_sample_set(), K.nan_directions()])
    ref, dbg = K.ref_samples(sky, d)
    ctx.rt_set_sky(sky)
    try:
        got = ctx.rt_sky_samples(d)
    finally:
        ctx.rt_set_sky(None)
    bad = np.argwhere((P.canonical_bits(got) != P.canonical_bits(ref)).any(-1))
    assert bad.size == 0, f"{len(bad)} of {len(d)} samples differ, first {bad[:4].ravel().tolist()}: {got[bad[0, 0]]} vs {ref[bad[0, 0]]}"
    assert set(dbg[:, 0].tolist()) == set(range(-1, 6)) and np.isnan(ref).any() and (ref[dbg[:, 0] < 0] == 0).all()


@pytest.mark.parametrize("sun", [K.SUN_UP, K.SUN_DOWN, K.elevated(80.0, 200.0)], ids=["low", "below-horizon", "high"])
def test_analytic_samples(ctx, sun):
    """The same directions (the finite, non-zero ones) into AnalyticSky: within helpers.TOL of the restatement, and on the
    restatement's branch.  The branch shows in the value: the disc is the constant (4, 3.5, 3) bit for bit, and a ring
    sample lies at mix(before, (3, 2.5, 1.5), edge), not at the colour before the branch (the numpy restatement gives both);
    the two are told apart wherever they differ by more than four tolerances."""
    sky = K.analytic_sky(sun)
    d = _sample_set()
    ref, dbg = K.ref_samples(sky, d)
    ok = np.isfinite(ref).all(-1)
    assert ok.sum() > len(d) - 200
    d, ref, branch = d[ok], ref[ok], dbg[ok, 0]
    ctx.rt_set_sky(sky)
    try:
        got = ctx.rt_sky_samples(d)
    finally:
        ctx.rt_set_sky(None)
    n_inexact = helpers.assert_float_close(got, ref, helpers.TOL, "analytic sky")
    is_disc = (_bits(got) == _bits(K.DISC)[None, :]).all(-1)
    assert np.array_equal(is_disc, branch == K.BRANCH_DISC), "the disc branch differs"
    _, _, _, _, before = K.np_analytic(sky.sun_dir, d)
    ring = branch == K.BRANCH_EDGE
    apart = np.abs(ref - before).max(-1) > 4 * helpers.TOL
    took_ring = np.abs(got - ref).max(-1) < np.abs(got - before).max(-1)
    assert took_ring[ring & apart].all() and (ring & ~apart).sum() <= 2, "the ring branch differs"
    if sun is K.SUN_UP:
        assert (branch == K.BRANCH_DISC).sum() > 20 and (ring & apart).sum() > 20
    print(f"analytic sky, sun {tuple(round(v, 3) for v in sun)}: {n_inexact} of {got.size} floats not bit-identical, "
          f"max difference {np.abs(got - ref).max():.3g}; {int(is_disc.sum())} disc and {int(ring.sum())} ring samples")


def test_samples_without_a_sky_are_rejected(ctx):
    import shs_gpu
    ctx.rt_set_sky(None)
    with pytest.raises(shs_gpu.ShsError) as e:
        ctx.rt_sky_samples([(0, 1, 0)])
    assert e.value.code == -1
    ctx.rt_set_sky(shs_gpu.RtSky(model=0))             # SHS_RT_SKY_NONE is no sky either
    with pytest.raises(shs_gpu.ShsError):
        ctx.rt_sky_samples([(0, 1, 0)])


# ---- whole frames -------------------------------------------------------------------------------------------

def check_frame(got, ref):
    """Every pixel of a frame against the restatement's planes: ids, depth and velocity bit-exact, colours under the parity
    rule with the pre-truncation floats within TOL * 255, the prequant plane's fourth float equal."""
    assert np.array_equal(got["tri_id"], ref["tri_id"])
    helpers.assert_depth_bitexact(got["depth"], ref["depth"])
    assert np.array_equal(_bits(got["velocity"]), _bits(ref["velocity"]))
    n = helpers.assert_color_parity(got["color"], ref["color"], got["prequant"], ref["prequant"])
    dp = np.abs(got["prequant"][..., :3] - ref["prequant"][..., :3])
    assert dp.max() <= helpers.TOL * 255.0, f"pre-truncation floats differ by {dp.max()}"
    assert np.array_equal(_bits(got["prequant"][..., 3]), _bits(ref["prequant"][..., 3]))
    return n, float(dp.max())


@pytest.mark.parametrize("size,via", [((W, H), "pbr"), ((161, 119), "hard")], ids=["160x120-pbr", "161x119-hard"])
@pytest.mark.parametrize("name", list(FRAME_SKIES))
def test_empty_frame_is_all_sky(ctx, name, size, via):
    """n_draws = 0 under each model and each encode: every pixel is sky; depth stays FLT_MAX, velocity 0, ids -1.
    161 x 119 is no multiple of the 256-lane block or of any tile shape."""
    sky = FRAME_SKIES[name]
    w, h = size
    view, lvp, _, _ = P.demo_scene()
    ref = K.ref_compose(sky, None, w, h)
    ref.update(depth=np.full((h, w), helpers.FLT_MAX, F), velocity=np.zeros((h, w, 2), F))
    ctx.rt_set_sky(sky)
    try:
        if via == "pbr":
            ctx.rt_render_pbr(P.pbr_frame(view, lvp, w, h, use_shadow=False), [], [])
        else:
            ctx.rt_render(R._frame(view, lvp, w, h, use_shadow=False), [])
        got = _planes(ctx)
    finally:
        ctx.rt_set_sky(None)
    assert (got["tri_id"] == -1).all() and (got["depth"] == helpers.FLT_MAX).all() and not got["velocity"].any()
    n, dp = check_frame(got, ref)
    assert (got["prequant"][..., 3] == 1).all() and (got["color"][..., 3] == 255).all()
    print(f"{name} {w}x{h}: {n} bytes off by one, max float difference {dp:.3g}")


DEMO_PATHS = [("pbr", (80, 80)), ("pbr", (160, 160)), ("pbr", (64, 48)), ("hard", (80, 80)), ("soft", (160, 160))]


def _render_demo(c, via, frame, draws, mats):
    if via == "pbr":
        c.rt_render_pbr(frame, draws, mats)
    else:
        c.rt_render(frame, draws)
    return _planes(c)


@pytest.mark.parametrize("via,tile", DEMO_PATHS, ids=[f"{v}-tile{t[0]}x{t[1]}" for v, t in DEMO_PATHS])
@pytest.mark.parametrize("name", list(DEMO_SKIES))
def test_demo_in_miniature(ctx, name, via, tile):
    """test_canvas_rt_pbr_ref.demo_scene, 160 x 120 over a 96^2 map, through shs_rt_render_pbr and through shs_rt_render with
    shading 0 and shading 1: with the sky bound, the pixels that show a fragment equal the sky-less frame's in every
    plane, bit for bit, and the whole frame equals the restatement's -- its pass, then the sky where no fragment is shown."""
    sky = DEMO_SKIES[name]
    view, lvp, draws, mats = P.demo_scene()
    ref_sm = R.ref_shadow(SM, lvp, draws, tile)
    shading = {"pbr": 2, "hard": 0, "soft": 1}[via]
    frame = R._frame(view, lvp, W, H, tile, shading=shading)
    if via == "pbr":
        plain = P.ref_render_pbr(frame, draws, mats, ref_sm, IBL)
    elif via == "soft":
        plain = S.ref_render_soft(frame, draws, ref_sm)
    else:
        plain = R.ref_render(frame, draws, ref_sm)
    ref = K.ref_compose(sky, plain)
    ctx.rt_set_ibl(*IBL)
    try:
        ctx.rt_render_shadow(SM, lvp, draws, ref_tile=tile)
        ctx.rt_set_sky(None)
        without = _render_demo(ctx, via, frame, draws, mats)
        ctx.rt_set_sky(sky)
        got = _render_demo(ctx, via, frame, draws, mats)
    finally:
        ctx.rt_set_sky(None)
        ctx.rt_set_ibl(None)
    covered = without["tri_id"] >= 0
    assert 3000 < covered.sum() < W * H - 3000
    for k in ("color", "depth", "velocity", "prequant", "tri_id"):
        assert np.array_equal(got[k][covered].view(np.uint8), without[k][covered].view(np.uint8)), f"{k}: a covered pixel changed"
    for k in ("depth", "velocity", "tri_id"):
        assert np.array_equal(got[k].view(np.uint8), without[k].view(np.uint8)), f"{k}: the background pass wrote it"
    clear = np.array(frame.clear_color, np.uint8)
    assert (without["color"][~covered] == clear).all() and (got["color"][~covered] != clear).any(-1).mean() > 0.99
    n, dp = check_frame(got, ref)
    if via == "pbr" and tile == (80, 80):
        # the C file's own composition of the whole PASS1 gives the same planes
        both = K.ref_render_pbr_sky(sky, frame, draws, mats, ref_sm, IBL)
        assert all(np.array_equal(both[k].view(np.uint8), ref[k].view(np.uint8)) for k in both)
    print(f"{name} through {via}, tile {tile}: {int((~covered).sum())} sky pixels, {n} bytes off by one, max float difference {dp:.3g}")


def test_no_sky_bound_is_the_parents_frame(ctx):
    """After shs_rt_set_sky(NULL) -- and after SHS_RT_SKY_NONE -- a frame is what it was before there was a sky: clear_color
    on the uncovered pixels, zeros in their prequant floats."""
    import shs_gpu
    view, lvp, draws, mats = P.demo_scene()
    ref_sm = R.ref_shadow(SM, lvp, draws)
    frame = P.pbr_frame(view, lvp)
    ref = P.ref_render_pbr(frame, draws, mats, ref_sm, IBL)
    ctx.rt_set_ibl(*IBL)
    try:
        ctx.rt_render_shadow(SM, lvp, draws)
        for unbind in (None, shs_gpu.RtSky(model=0)):
            ctx.rt_set_sky(DEMO_SKIES["analytic"])
            ctx.rt_render_pbr(frame, draws, mats)
            assert (_planes(ctx)["color"][ref["tri_id"] < 0] != np.array(frame.clear_color, np.uint8)).any()
            ctx.rt_set_sky(unbind)
            ctx.rt_render_pbr(frame, draws, mats)
            got = _planes(ctx)
            check_frame(got, ref)
            open_px = ref["tri_id"] < 0
            assert (got["color"][open_px] == np.array(frame.clear_color, np.uint8)).all() and not got["prequant"][open_px].any()
    finally:
        ctx.rt_set_sky(None)
        ctx.rt_set_ibl(None)


def test_rejected_calls_keep_the_bound_sky():
    import shs_gpu
    nan, inf = float("nan"), float("inf")
    view, lvp, _, _ = P.demo_scene()
    frame = R._frame(view, lvp, 33, 31, use_shadow=False)
    good = FRAME_SKIES["analytic-reinhard"]
    cube = FRAME_SKIES["cubemap-clamp"]
    with shs_gpu.Context(0) as c:
        ids = tuple(c.upload_texture(t) for t in cube.face_tex)
        bad = [
            ("model 3", dataclasses.replace(good, model=3)), ("model -1", dataclasses.replace(good, model=-1)),
            ("encode 2", dataclasses.replace(good, encode=2)), ("encode -1", dataclasses.replace(cube, encode=-1)),
            ("NaN sun", dataclasses.replace(good, sun_dir=(nan, 0.0, 1.0))), ("infinite intensity", dataclasses.replace(cube, intensity=inf)),
            ("NaN fov", dataclasses.replace(good, fov_degrees=nan)), ("infinite exposure", dataclasses.replace(good, exposure=-inf)),
            ("NaN camera", dataclasses.replace(good, cam_up=(0.0, nan, 0.0))), ("zero forward", dataclasses.replace(good, cam_forward=(0.0, 0.0, 0.0))),
            ("zero right", dataclasses.replace(cube, cam_right=(0.0, 0.0, 0.0))), ("zero up", dataclasses.replace(good, cam_up=(0.0, -0.0, 0.0))),
            ("zero sun", dataclasses.replace(good, sun_dir=(0.0, 0.0, 0.0))),
            ("face id 0", dataclasses.replace(cube, face_tex=ids[:5] + (0,))), ("face id 999", dataclasses.replace(cube, face_tex=(999,) + ids[1:])),
            ("face id -1", dataclasses.replace(cube, face_tex=ids[:2] + (-1,) + ids[3:])), ("five faces", dataclasses.replace(cube, face_tex=ids[:5])),
        ]
        for bound, ref_sky in ((good, good), (dataclasses.replace(cube, face_tex=ids), cube)):
            c.rt_set_sky(bound)
            c.rt_render(frame, [])
            before = _planes(c)
            check_frame(before, dict(K.ref_compose(ref_sky, None, 33, 31), depth=before["depth"], velocity=before["velocity"]))
            for what, sky in bad:
                with pytest.raises(shs_gpu.ShsError) as e:
                    c.rt_set_sky(sky)
                assert e.value.code == -1, what
                c.rt_render(frame, [])
                after = _planes(c)
                assert all(np.array_equal(after[k].view(np.uint8), before[k].view(np.uint8)) for k in before), f"{what}: the bound sky changed"
                if ref_sky.model == K.CUBEMAP:          # (bit-exact: shs_rt_sky_samples still samples the bound cubemap)
                    assert np.array_equal(_bits(c.rt_sky_samples([(0.1, 0.5, 1.0)])), _bits(K.ref_samples(ref_sky, [(0.1, 0.5, 1.0)])[0]))
        # a face of the bound cubemap cannot be released; once another sky is bound it can
        assert c._lib.shs_texture_release(c._h, ids[2]) != 0
        c.rt_set_sky(good)
        assert c._lib.shs_texture_release(c._h, ids[2]) == 0
