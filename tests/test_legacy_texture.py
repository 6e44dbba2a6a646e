"""The texture-mapping pipeline (SHADING_TEXTURED) of the legacy raster on the GPU against
tests/legacy_texture_ref (test_legacy_texture_ref.py holds the wrapper, the scenes and what pins the reference
on the CPU).

Per frame: depth and coverage bit-exact, the texel index of every covered textured pixel equal (the
textures' colours code their texel, texel_of_prequant), colours through helpers.assert_color_parity as it
stands with helpers.TOL on the pre-truncation floats -- no pixel is excused.

Frames: Scenes A (the monkey with its UVs), B (the grazing ground quad, UVs -0.25 .. 1.25, 2x3 and 1x1
textures) and C (one corner behind the camera: the invw_sum <= 0 skip) in scan and bin mode with tile groups
on and off, plus the row-span, per-pixel and pipelined variants; a frame mixing three textured draws with
Blinn-Phong and Toon; a batch of two poses; two shards; a one-device group; PRESENT; a mesh without UVs, a
draw without a texture, a shared mesh.  Then the sampler's edge sets, the rejections, a texture released right
after the render call, and a Blinn-Phong frame through the textured entry point."""
import copy
import ctypes

import numpy as np
import pytest

import helpers
import test_legacy_shaders_ref as shaders_ref
from test_legacy_texture_ref import (BLINN, CAM, COLOR, F, H, LIGHT, TEX_A, TEXTURED, W, _draw, coded_texture,
                                     covered, ref_render, ref_sample, sampler_sets, scene_a, scene_frame, texel_of_prequant,
                                     texture_of, two_triangle_draws)

pytestmark = pytest.mark.gpu
TOON = shaders_ref.TOON

# raster variants: option setters per context (scan mode 1, bin mode 2)
VARIANTS = {
    "scan": dict(mode=1),                                  # tile groups with row spans (batches)
    "scan_boxes": dict(mode=1, group_spans=False),         # tile groups, whole boxes
    "tiles": dict(mode=1, tile_groups=False),              # a work item per tile
    "bins": dict(mode=2),                                  # binned, tile row spans (tile groups do not apply)
    "bins_tiles": dict(mode=2, tile_groups=False),
    "pixel": dict(mode=1, loop=0),                         # the per-pixel loop
    "pixel_bins": dict(mode=2, loop=0),
    "pipe": dict(mode=1, pipeline=True),                   # k_pipe (batches of more than six draws)
}


@pytest.fixture(scope="module")
def ctxs():
    import shs_gpu
    cs = {}
    for name, o in VARIANTS.items():
        c = shs_gpu.Context(0)
        c.set_raster_mode(o["mode"])
        if "tile_groups" in o:
            c.set_tile_groups(o["tile_groups"])
        if "group_spans" in o:
            c.set_group_spans(o["group_spans"])
        if "loop" in o:
            c.set_raster_loop(o["loop"])
        if o.get("pipeline"):
            c.set_legacy_pipeline(True)
        cs[name] = c
    yield cs
    for c in cs.values():
        c.close()


def frame_desc(**kw):
    import shs_gpu
    return shs_gpu.Frame(W, H, prequant=True, **kw)


def _planes(ctx, k=0):
    color, depth = ctx.resolve_frame(k)
    return {"color": color, "depth": depth, "prequant": ctx.resolve_prequant(k)}


def _check_textured(got, ref, draws, mine=None):
    """got against the texture reference's planes on the pixels `mine` (default: all it covers)."""
    if mine is None:
        mine = covered(ref)
        helpers.assert_depth_bitexact(got["depth"], ref["depth"])
        assert np.array_equal(got["color"][..., 3], ref["color"][..., 3])
    for i, d in enumerate(draws):
        px = mine & (ref["draw_id"] == i)
        if d.shading != TEXTURED or texture_of(d) is None or not px.any():
            continue
        idx = texel_of_prequant(texture_of(d), got["prequant"])
        bad = px & (idx != ref["texel"])
        assert not bad.any(), f"draw {i}: {int(bad.sum())} of {int(px.sum())} pixels sampled another texel"
    m = mine[..., None]
    g_c, r_c = np.where(m, got["color"], 0), np.where(m, ref["color"], 0)
    g_p, r_p = np.where(m, got["prequant"], 0), np.where(m, ref["prequant"], 0)
    helpers.assert_color_parity(g_c, r_c, g_p, r_p)
    dp = np.abs(g_p[..., :3] - r_p[..., :3])
    assert dp.max() <= helpers.TOL * 255.0, f"pre-truncation floats differ by {dp.max()}"


@pytest.mark.parametrize("variant", ["scan", "scan_boxes", "tiles", "bins", "bins_tiles", "pixel", "pixel_bins"])
@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_scene(ctxs, name, variant):
    """Two frames of the scene in one batch (so that the scan contexts run tile groups), then one alone."""
    draws, ref = scene_frame(name)
    c = ctxs[variant]
    c.render_batch(frame_desc(), [draws, draws])
    for k in range(2):
        _check_textured(_planes(c, k), ref, draws)
    c.render(frame_desc(), draws)
    assert c.stats()["covered_pixels"] == int(covered(ref).sum())
    _check_textured(_planes(c), ref, draws)
    if name == "C":   # the skipped pixels are absent from depth and colour: the reference dropped hundreds
        assert ref["skipped"] > 300


# ---- the mixed frame ------------------------------------------------------------------------------------
MIXED_POS = [(-5.0, -1.0, 10.5), (-2.5, 1.5, 10.0), (0.0, -1.5, 10.5), (2.5, 1.5, 10.0), (5.0, -1.0, 10.5)]
MIXED_SCALE = 3.5
TEX_M = coded_texture(5, 4, 10, 20, 10, 25)


def _mixed_draws():
    from shs_gpu import scene
    view, proj = scene.camera(CAM, 0.0, 0.0)
    kinds = [(TEXTURED, TEX_A), (BLINN, None), (TEXTURED, TEX_M), (TOON, None), (TEXTURED, 0)]
    draws = []
    for (shading, tex), pos in zip(kinds, MIXED_POS):
        model = scene.model_trs(pos, -30.0, (MIXED_SCALE, MIXED_SCALE, MIXED_SCALE))
        draws.append(_draw(scene.monkey(), model, view, proj, CAM, tex, shaders_ref.COLOR if shading != TEXTURED else COLOR, shading))
    return draws


def _mixed_reference(draws):
    """Each draw alone in its own reference -- the texture reference for model 9, the shaders' reference (whose
    Blinn-Phong is pinned against the oracle) for the others -- composed as the shared ZBuffer would: the
    smallest depth, the earlier draw on a tie (test_and_set_depth is a strict '<' in submission order)."""
    out = {"color": np.zeros((H, W, 4), np.uint8), "depth": np.full((H, W), helpers.FLT_MAX, F),
           "prequant": np.zeros((H, W, 4), F), "draw_id": np.full((H, W), -1, np.int32), "texel": np.full((H, W), -1, np.int32),
           "spec_margin": np.full((H, W), np.inf, F), "cos_beta": np.full((H, W), np.inf, F)}
    out["color"][..., 3] = 255
    for i, d in enumerate(draws):
        one = ref_render(W, H, [d]) if d.shading == TEXTURED else shaders_ref.ref_render(W, H, [d])
        win = one["depth"] < out["depth"]        # screen rows
        out["depth"] = np.where(win, one["depth"], out["depth"])
        wc = win[::-1]                           # canvas rows
        out["color"] = np.where(wc[..., None], one["color"], out["color"])
        out["prequant"] = np.where(wc[..., None], one["prequant"], out["prequant"])
        out["draw_id"] = np.where(wc, i, out["draw_id"])
        for k in ("texel", "spec_margin", "cos_beta"):
            if k in one:
                out[k] = np.where(wc, one[k], out[k])
            else:
                out[k] = np.where(wc, -1 if k == "texel" else np.inf, out[k]).astype(out[k].dtype)
    return out


@pytest.mark.parametrize("variant", ["scan", "tiles", "bins", "pipe"])
def test_mixed_frame_with_blinn_phong_and_toon(ctxs, variant):
    draws = _mixed_draws()
    ref = _mixed_reference(draws)
    for i in range(5):
        assert (ref["draw_id"] == i).sum() > 150, i
    c = ctxs[variant]
    c.render_batch(frame_desc(), [draws, draws])   # (ten draws: the pipelined context takes k_pipe's path)
    for k in range(2):
        got = _planes(c, k)
        helpers.assert_depth_bitexact(got["depth"], ref["depth"])
        assert np.array_equal(got["color"][..., 3], ref["color"][..., 3])
        tex_px = np.isin(ref["draw_id"], [0, 2, 4])
        _check_textured(got, ref, draws, mine=tex_px)
        for i, model in ((1, BLINN), (3, TOON)):
            mine = ref["draw_id"] == i
            skip = shaders_ref.excusable(model, ref) & mine
            assert int(skip.sum()) <= shaders_ref.CAP * int(mine.sum())
            judge = (mine & ~skip)[..., None]
            helpers.assert_color_parity(np.where(judge, got["color"], 0), np.where(judge, ref["color"], 0),
                                        np.where(judge, got["prequant"], 0), np.where(judge, ref["prequant"], 0))
    if variant == "pipe":   # a batch without model 9 behind a pending textured one, and back
        plain = [copy.copy(d) for d in draws]
        for d in plain:
            d.shading, d.albedo_tex = BLINN, None
        c.render_batch(frame_desc(), [plain, plain])
        c.render_batch(frame_desc(), [draws, draws])
        helpers.assert_depth_bitexact(_planes(c, 1)["depth"], ref["depth"])


def test_batch_of_two_poses(ctxs):
    poses = [dict(cam_pos=(0.0, 5.0, -20.0)), dict(cam_pos=(3.0, 4.0, -19.0), yaw=6.0)]
    fds = [scene_a(**p) for p in poses]
    for variant in ("scan", "bins"):
        c = ctxs[variant]
        c.render_batch(frame_desc(), fds)
        for k in range(2):
            _check_textured(_planes(c, k), ref_render(W, H, fds[k]), fds[k])


def test_two_shards_make_the_unsharded_frame(ctxs):
    draws, ref = scene_frame("B")
    T = 32                          # rank r owns the 32x32 tiles t with t % 2 == r, row-major
    tx, ty = (W + T - 1) // T, (H + T - 1) // T
    color = np.zeros((H, W, 4), np.uint8)
    depth = np.zeros((H, W), F)
    pq = np.zeros((H, W, 4), F)
    c = ctxs["scan"]
    for r in range(2):
        c.render(frame_desc(shard_rank=r, shard_count=2), draws)
        part = _planes(c)
        for t in range(r, tx * ty, 2):
            x0, y0 = (t % tx) * T, (t // tx) * T
            x1, y1 = min(x0 + T, W), min(y0 + T, H)
            depth[y0:y1, x0:x1] = part["depth"][y0:y1, x0:x1]
            color[H - y1:H - y0, x0:x1] = part["color"][H - y1:H - y0, x0:x1]
            pq[H - y1:H - y0, x0:x1] = part["prequant"][H - y1:H - y0, x0:x1]
    _check_textured({"color": color, "depth": depth, "prequant": pq}, ref, draws)


def test_one_device_group_and_present(ctxs):
    from shs_gpu.group import Group
    draws, ref = scene_frame("A")
    frame = frame_desc(present=True)
    single = ctxs["scan"]
    single.render(frame, draws)
    want = single.resolve_present(0)
    got = _planes(single)
    _check_textured(got, ref, draws)
    assert np.array_equal(want, got["color"][::-1])   # PRESENT: the colour plane's pixels, rows top-down
    g = Group([0])
    try:
        g.render(frame, draws)
        g.gather(single.TARGET_PRESENT)
        assert np.array_equal(g.root.resolve_present(0), want)
    finally:
        g.close()


def test_mesh_without_uvs_and_draw_without_texture(ctxs):
    """The CPU test's two-triangle frames: a mesh uploaded without UVs reads vec2(0) per corner (texel 0), a
    textured draw without a texture takes Uniforms::color."""
    for name, draws in two_triangle_draws().items():
        ref = ref_render(W, H, draws)
        for variant in ("tiles", "bins"):
            c = ctxs[variant]
            c.render(frame_desc(), draws)
            _check_textured(_planes(c), ref, draws)


def test_shared_mesh_keeps_its_uvs(ctxs):
    draws, ref = scene_frame("A")
    src, dst = ctxs["tiles"], ctxs["scan"]
    sid = src.upload_mesh(draws[0].mesh)
    mid = ctypes.c_int32()
    dst._check(dst._lib.shs_mesh_share(dst._h, src._h, sid, ctypes.byref(mid)))
    d = copy.copy(draws[0])
    d.mesh = mid.value
    dst.render(frame_desc(), [d])
    _check_textured(_planes(dst), ref, draws)
    dst._check(dst._lib.shs_mesh_release(dst._h, mid.value))


# ---- the sampler, the rejections, release ---------------------------------------------------------------
def test_sample_nearest_edge_sets(ctxs):
    c = ctxs["scan"]
    for tex, uv, _ in sampler_sets():
        rgba, _ = ref_sample(tex, uv)
        assert np.array_equal(c.legacy_sample_nearest(tex, uv), rgba)


def test_rejections(ctxs):
    import shs_gpu
    c = ctxs["scan"]
    draws = scene_frame("A")[0]
    bad = copy.copy(draws[0])
    bad.albedo_tex = 9999
    with pytest.raises(shs_gpu.ShsError, match="bad texture id"):
        c.render(frame_desc(), [bad])
    with pytest.raises(shs_gpu.ShsError, match="bad texture id"):
        c.legacy_sample_nearest(9999, [(0.5, 0.5)])
    one = np.ones((1, 3), F)
    with pytest.raises(shs_gpu.ShsError, match="bad shading model"):
        c.legacy_shade_samples(TEXTURED, LIGHT, CAM, COLOR, one, one, [0.0])
    # the untextured render call takes the models it has always taken: a textured draw none of whose batch
    # sets albedo_tex goes there, and is answered like any model that call does not know
    plain = copy.copy(draws[0])
    plain.albedo_tex = None
    with pytest.raises(shs_gpu.ShsError, match="bad shading model"):
        c.render(frame_desc(), [plain])
    with pytest.raises(shs_gpu.ShsError, match="bad shading model"):
        c.render_batch(frame_desc(), [[plain], [plain]])
    # an unknown id on a draw of another model is not read
    other = copy.copy(draws[0])
    other.shading, other.albedo_tex = BLINN, 9999
    c.render(frame_desc(), [other])


def test_release_texture_right_after_render(ctxs):
    import shs_gpu
    draws, ref = scene_frame("A")
    for variant in ("scan", "pipe"):
        c = ctxs[variant]
        tid = ctypes.c_int32()
        rgba = TEX_A.rgba
        c._check(c._lib.shs_texture_upload(c._h, rgba.ctypes.data_as(ctypes.c_void_p), rgba.shape[1], rgba.shape[0], ctypes.byref(tid)))
        d = copy.copy(draws[0])
        d.albedo_tex = tid.value
        c.render_batch(frame_desc(), [[d] * 4, [d] * 4])   # (eight draws: pending on the pipelined context)
        c.release_texture(tid.value)
        got = _planes(c, 1)
        helpers.assert_depth_bitexact(got["depth"], ref["depth"])
        helpers.assert_color_parity(got["color"], ref["color"], got["prequant"], ref["prequant"])
        with pytest.raises(shs_gpu.ShsError):
            c.release_texture(tid.value)


def test_blinn_phong_through_the_textured_entry_point(ctxs):
    """shs_render_legacy_batch_tex with albedo_tex NULL is shs_render_legacy_batch, byte for byte."""
    draws = [shaders_ref.monkey_draw(BLINN), shaders_ref.monkey_draw(BLINN, position=(2.0, 1.0, 13.0), scale=3.0)]
    c = ctxs["scan"]
    prepared = c.prepare_batch(frame_desc(), [draws, draws])
    frame, desc, arr, n, n_frames = prepared
    assert getattr(arr, "albedo_tex", None) is None
    c.render_batch_prepared(prepared)
    want = [_planes(c, k) for k in range(2)]
    c._check(c._lib.shs_render_legacy_batch_tex(c._h, ctypes.byref(desc), arr, None, n, n_frames))
    for k in range(2):
        got = _planes(c, k)
        assert np.array_equal(got["depth"].view(np.uint32), want[k]["depth"].view(np.uint32))
        assert np.array_equal(got["color"], want[k]["color"])
        assert np.array_equal(got["prequant"].view(np.uint32), want[k]["prequant"].view(np.uint32))
    assert (want[0]["color"][..., :3] != 0).any()
