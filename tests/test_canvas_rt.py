"""The Canvas render-target raster on the GPU (shs_rt_render_shadow, shs_rt_render) against tests/canvas_rt_ref
(test_canvas_rt_ref.py holds the wrapper, the scenes and what pins the reference on the CPU).

Per frame, on every pixel, none excused: the shadow map, the view-z depth, the velocity and the shadow factor
(the prequant plane's alpha) bit-exact; the shading sub-triangle equal; the texel index of every textured pixel
equal (the texture's colours code their texel); colours through helpers.assert_color_parity with the
pre-truncation floats; the setup counters equal."""
import ctypes
import dataclasses

import numpy as np
import pytest

import helpers
import test_canvas_rt_ref as R
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


def _draw_of(draws, tri_id):
    """The draw each sub-triangle id belongs to (-1 where none)."""
    ends = np.cumsum([d.mesh.positions.shape[0] for d in draws])
    return np.where(tri_id >= 0, np.searchsorted(ends, tri_id // 2, side="right"), -1)


def check_camera(c, frame, draws, ref, gpu_draws=None):
    c.rt_render(frame, draws if gpu_draws is None else gpu_draws)
    color, depth, vel = c.rt_resolve()
    pq, ids = c.rt_resolve_prequant(), c.rt_resolve_ids()
    helpers.assert_depth_bitexact(depth, ref["depth"])
    bad = np.argwhere(ids != ref["tri_id"])
    assert bad.size == 0, f"{len(bad)} pixels shaded by another sub-triangle, first {bad[:4].tolist()}"
    bad = np.argwhere((_bits(vel) != _bits(ref["velocity"])).any(-1))
    assert bad.size == 0, f"{len(bad)} velocities differ, first {bad[:4].tolist()}"
    bad = np.argwhere(_bits(pq[..., 3]) != _bits(ref["prequant"][..., 3]))
    assert bad.size == 0, f"{len(bad)} shadow factors differ, first {bad[:4].tolist()}"
    who = _draw_of(draws, ref["tri_id"])
    for i, d in enumerate(draws):
        if d.albedo_tex is None:
            continue
        px = who == i
        idx = R.texel_of_prequant(d.albedo_tex, pq)
        wrong = px & (idx != ref["texel"])
        assert not wrong.any(), f"draw {i}: {int(wrong.sum())} of {int(px.sum())} pixels sampled another texel"
    helpers.assert_color_parity(color, ref["color"], pq, ref["prequant"])
    dp = np.abs(pq[..., :3] - ref["prequant"][..., :3])
    assert dp.max() <= helpers.TOL * 255.0, f"pre-truncation floats differ by {dp.max()}"
    assert c.rt_stats() == ref["counters"]
    return color, depth, vel


def check_both(c, view, lvp, draws, w=W, h=H, sm=SM, tile=(80, 80), **kw):
    ref_sm = R.ref_shadow(sm, lvp, draws, tile)
    c.rt_render_shadow(sm, lvp, draws, ref_tile=tile)
    got_sm = c.rt_resolve_shadow()
    bad = np.argwhere(_bits(got_sm) != _bits(ref_sm))
    assert bad.size == 0, f"{len(bad)} shadow-map texels differ, first {bad[:4].tolist()}"
    frame = R._frame(view, lvp, w, h, tile, **kw)
    ref = R.ref_render(frame, draws, ref_sm if frame.use_shadow else None)
    return check_camera(c, frame, draws, ref), ref


@pytest.mark.parametrize("pcf,use_shadow,tile", [(True, True, 80), (False, True, 80), (True, False, 80), (True, True, 160)],
                         ids=["pcf", "compare", "no-map", "tile160"])
def test_demo_in_miniature(ctx, pcf, use_shadow, tile):
    view, lvp, draws = R.scene_demo()
    check_both(ctx, view, lvp, draws, tile=(tile, tile), pcf=pcf, use_shadow=use_shadow)


@pytest.mark.parametrize("name", ["windings", "near", "coincident", "outside"])
def test_scene(ctx, name):
    """Both windings drawn; the near-plane set; coincident triangles (the first wins, ids 2 t + k); receivers and
    casters outside the light's box.  test_canvas_rt_ref.py asserts each shows its phenomenon in the reference."""
    view, lvp, draws = R.SCENES[name]()
    check_both(ctx, view, lvp, draws)


@pytest.mark.parametrize("tile", [(80, 80), (R.HAIR_W, R.HAIR_H)], ids=["tile80", "one-tile"])
def test_hair_slivers(ctx, tile):
    """Slivers whose float barycentrics pass outside their own bbox, where only the reference's tile clamp visits
    them: both passes equal the reference against 80-pixel jobs and against one job."""
    view, lvp, draws = R.scene_hair()
    check_both(ctx, view, lvp, draws, w=R.HAIR_W, h=R.HAIR_H, sm=(R.HAIR_W, R.HAIR_H), tile=tile, use_shadow=False)


def test_frame_size_sequence(ctx):
    """1x1, 33x31 and 160x120 through one context, the shadow map resized in between."""
    for (w, h), sm in [((1, 1), 8), ((33, 31), 50), ((160, 120), 96), ((33, 31), 8)]:
        view, proj = R.camera(w, h)
        _, lvp, draws = R.scene_demo()
        draws = [R._rt_draw(d.mesh, d.model, view, proj, color=d.base_color, tex=d.albedo_tex) for d in draws]
        check_both(ctx, view, lvp, draws, w=w, h=h, sm=sm)


def test_end_to_end_on_the_device(ctx, oracle_mod):
    """PASS0, PASS1, then shs_rt_device_targets into shs_canvas_motion_blur(SHS_CANVAS_DEVICE): equal, byte for
    byte, to the oracle's pass over the restatement's planes."""
    import torch
    from shs_gpu import _abi
    view, lvp, draws = R.scene_demo()
    _, proj = R.camera()
    ctx._on_torch_stream()
    (color, depth, vel), ref = check_both(ctx, view, lvp, draws)
    ctx.rt_render(R._frame(view, lvp), draws)
    c_dev, d_dev, v_dev = ctx.rt_device_targets()
    dst = torch.empty((H, W, 4), dtype=torch.uint8, device="cuda")
    d = _abi.CanvasMotionBlurDescC()
    d.width, d.height = W, H
    for k in range(16):
        d.curr_view[k] = d.prev_view[k] = float(view[k])
        d.curr_proj[k] = d.prev_proj[k] = float(proj[k])
    d.samples, d.strength, d.w_obj, d.w_cam, d.soft_knee, d.knee_px, d.max_px = 12, 0.85, 1.0, 0.35, 1, 18.0, 22.0
    _P = ctypes.c_void_p
    ctx._check(ctx._lib.shs_canvas_motion_blur(ctx._h, ctypes.byref(d), _P(c_dev), _P(d_dev), _P(v_dev), _P(dst.data_ptr()),
                                               ctx.CANVAS_DEVICE))
    ctx.synchronize()
    got = dst.cpu().numpy()
    want = oracle_mod.canvas_motion_blur(ref["color"], ref["depth"], ref["velocity"], view, proj, view, proj)
    bad = np.argwhere((got != want).any(-1))
    assert bad.size == 0, f"{len(bad)} pixels differ, first {bad[:4].tolist()}"
    assert (got != ref["color"]).any()


def test_rejections():
    import shs_gpu
    view, lvp, draws = R.scene_windings()
    with shs_gpu.Context(0) as c:
        frame = R._frame(view, lvp)
        with pytest.raises(shs_gpu.ShsError) as e:      # no shadow map rendered yet
            c.rt_render(frame, draws)
        assert e.value.code == -1
        bad_mesh = [dataclasses.replace(draws[0], mesh=999)]
        bad_tex = [dataclasses.replace(draws[0], albedo_tex=77)]
        for call in (lambda: c.rt_render_shadow(SM, lvp, bad_mesh), lambda: c.rt_render_shadow((0, 8), lvp, draws),
                     lambda: c.rt_render_shadow(SM, lvp, draws, ref_tile=(0, 80))):
            with pytest.raises(shs_gpu.ShsError) as e:
                call()
            assert e.value.code == -1
        c.rt_render_shadow(SM, lvp, draws)
        for fr, dr in ((frame, bad_mesh), (frame, bad_tex), (dataclasses.replace(frame, width=0), draws),
                       (dataclasses.replace(frame, ref_tile=(80, -1)), draws)):
            with pytest.raises(shs_gpu.ShsError) as e:
                c.rt_render(fr, dr)
            assert e.value.code == -1
        with pytest.raises(shs_gpu.ShsError):           # nothing rendered: nothing to resolve
            c.rt_resolve()
        c.rt_render(frame, draws)                       # the context still renders after the rejections
        assert (c.rt_resolve_ids() >= 0).sum() > 1000


def test_release_right_after_the_render_call():
    """A texture and a mesh released as soon as the calls return: the release finishes the frame in flight."""
    import shs_gpu
    view, lvp, draws = R.scene_demo()
    ref_sm = R.ref_shadow(SM, lvp, draws)
    frame = R._frame(view, lvp)
    ref = R.ref_render(frame, draws, ref_sm)
    with shs_gpu.Context(0) as c:
        ids = [c.upload_soup(d.mesh.positions, d.mesh.normals, d.mesh.uvs) for d in draws]
        tex = c.upload_texture(R.coded_texture(16, 12, 10, 5, 10, 7))
        gpu_draws = [dataclasses.replace(d, mesh=m, albedo_tex=None if d.albedo_tex is None else tex) for d, m in zip(draws, ids)]
        c.rt_render_shadow(SM, lvp, gpu_draws)
        c.rt_render(frame, gpu_draws)
        c.release_texture(tex)
        for m in ids:
            c._check(c._lib.shs_mesh_release(c._h, m))
        assert np.array_equal(_bits(c.rt_resolve_shadow()), _bits(ref_sm))
        color, depth, vel = c.rt_resolve()
        helpers.assert_depth_bitexact(depth, ref["depth"])
        assert np.array_equal(c.rt_resolve_ids(), ref["tri_id"])
        pq = c.rt_resolve_prequant()
        helpers.assert_color_parity(color, ref["color"], pq, ref["prequant"])
        with pytest.raises(shs_gpu.ShsError):           # the ids are gone
            c.rt_render(frame, gpu_draws)
