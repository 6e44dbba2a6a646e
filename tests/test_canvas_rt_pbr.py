"""The GGX + IBL camera pass on the GPU (shs_rt_render_pbr, shs_rt_set_pbr, shs_rt_set_ibl, shs_rt_ibl_samples) against
tests/canvas_rt_pbr_ref (test_canvas_rt_pbr_ref.py holds the wrapper, the materials, the IBLs, the sample sets and what
pins the reference on the CPU; the scenes and the camera are test_canvas_rt_ref's).

Per frame, on every pixel, none excused (check_pbr): the view-z depth, the velocity and the shadow factor (the prequant
plane's alpha) bit-exact; the shading sub-triangle equal; the texel index of every textured pixel equal; colours
through helpers.assert_color_parity with the pre-truncation floats within helpers.TOL * 255; the setup counters equal.
PASS0 is the hard demo's and is compared as there.

The texel: the shader's output is a strictly increasing function of each base-colour byte once the light's intensity is
0 and no IBL is set -- it is then encode(lin(byte) * 0.03 * ao * exposure) -- so a second frame of the same pass under
those constants (exposure 1000, which spreads the texture's bytes 10 .. 87 over 46 .. 221 of the output, neighbouring
codes at least 3.8 apart) gives back the bytes the kernel sampled, and with them the texel the coded texture encodes."""
import ctypes
import dataclasses

import numpy as np
import pytest

import helpers
import test_canvas_rt as T
import test_canvas_rt_pbr_ref as P
import test_canvas_rt_ref as R
import test_canvas_rt_soft_ref as S
from test_canvas_rt_ref import F, H, SM, W

pytestmark = pytest.mark.gpu
IBL = P.make_ibl()          # irradiance 4^2, specular 8, 4, 2, 1
DECODE = dict(exposure=1000.0, direct_intensity=0.0)


@pytest.fixture(scope="module")
def ctx():
    import shs_gpu
    c = shs_gpu.Context(0)
    yield c
    c.close()


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _set(c, ibl, consts):
    if ibl is None:
        c.rt_set_ibl(None)
    else:
        c.rt_set_ibl(*ibl)
    c.rt_set_pbr(consts)


def _sampled_texels(c, frame, draws, mats, who):
    """{draw index: the texel index each of its pixels sampled}, from a frame under DECODE (module docstring)."""
    if all(d.albedo_tex is None for d in draws):
        return {}
    _set(c, None, P.demo_consts(**DECODE))
    c.rt_render_pbr(dataclasses.replace(frame, use_shadow=False), draws, mats)
    pq = c.rt_resolve_prequant().astype(np.float64)
    lin = (np.arange(256) / 255.0) ** 2.2
    out = {}
    for i, d in enumerate(draws):
        if d.albedo_tex is None:
            continue
        ao = min(max(float(mats[i].ao), 0.0), 1.0)
        assert ao > 0
        x = lin * 0.03 * ao * DECODE["exposure"]
        table = 255.0 * (x / (1.0 + x)) ** (1.0 / 2.2)
        px = who == i
        byte = [np.abs(pq[px][:, k, None] - table[None, :]).argmin(axis=1) for k in (0, 1)]
        r0, rs, g0, gs = d.albedo_tex.code
        tx, ty = (byte[0] - r0) / rs, (byte[1] - g0) / gs
        assert (tx == np.rint(tx)).all() and (ty == np.rint(ty)).all(), f"draw {i}: bytes that are no texel's code"
        out[i] = (ty * d.albedo_tex.rgba.shape[1] + tx).astype(np.int64)
    return out


def check_camera_pbr(c, frame, draws, mats, ref, ibl, consts):
    """What test_canvas_rt.check_camera checks, through rt_render_pbr."""
    _set(c, ibl, consts)
    c.rt_render_pbr(frame, draws, mats)
    color, depth, vel = c.rt_resolve()
    pq, ids = c.rt_resolve_prequant(), c.rt_resolve_ids()
    helpers.assert_depth_bitexact(depth, ref["depth"])
    bad = np.argwhere(ids != ref["tri_id"])
    assert bad.size == 0, f"{len(bad)} pixels shaded by another sub-triangle, first {bad[:4].tolist()}"
    bad = np.argwhere((_bits(vel) != _bits(ref["velocity"])).any(-1))
    assert bad.size == 0, f"{len(bad)} velocities differ, first {bad[:4].tolist()}"
    bad = np.argwhere(_bits(pq[..., 3]) != _bits(ref["prequant"][..., 3]))
    assert bad.size == 0, f"{len(bad)} shadow factors differ, first {bad[:4].tolist()}"
    n = helpers.assert_color_parity(color, ref["color"], pq, ref["prequant"])
    dp = np.abs(pq[..., :3] - ref["prequant"][..., :3])
    assert dp.max() <= helpers.TOL * 255.0, f"pre-truncation floats differ by {dp.max()}"
    assert c.rt_stats() == ref["counters"]
    who = T._draw_of(draws, ref["tri_id"])
    for i, idx in _sampled_texels(c, frame, draws, mats, who).items():
        want = ref["texel"][who == i]
        wrong = idx != want
        assert not wrong.any(), f"draw {i}: {int(wrong.sum())} of {len(want)} pixels sampled another texel"
    exact = int((_bits(pq[..., :3]) != _bits(ref["prequant"][..., :3])).sum())
    print(f"pbr frame {frame.width}x{frame.height}: {exact} of {3 * int((ids >= 0).sum())} colour floats not bit-identical, "
          f"{n} bytes off by one, max float difference {dp.max():.3g}")
    return color, depth, vel


def check_pbr(c, view, lvp, draws, mats, w=W, h=H, sm=SM, tile=(80, 80), ibl=IBL, consts=None, **kw):
    """Both passes against the restatements -> ((color, depth, velocity), the reference's planes)."""
    ref_sm = R.ref_shadow(sm, lvp, draws, tile)
    c.rt_render_shadow(sm, lvp, draws, ref_tile=tile)
    bad = np.argwhere(_bits(c.rt_resolve_shadow()) != _bits(ref_sm))
    assert bad.size == 0, f"{len(bad)} shadow-map texels differ, first {bad[:4].tolist()}"
    frame = P.pbr_frame(view, lvp, w, h, tile, **kw)
    ref = P.ref_render_pbr(frame, draws, mats, ref_sm if frame.use_shadow else None, ibl, consts)
    try:
        got = check_camera_pbr(c, frame, draws, mats, ref, ibl, consts)
    finally:
        _set(c, None, None)
    return got, ref


@pytest.mark.parametrize("tile", [(80, 80), (160, 160), (64, 48)], ids=["tile80", "tile160", "tile64x48"])
@pytest.mark.parametrize("pcf", [True, False], ids=["pcf", "compare"])
@pytest.mark.parametrize("use_shadow", [True, False], ids=["map", "no-map"])
def test_demo_in_miniature(ctx, use_shadow, pcf, tile):
    """160 x 120 over a 96^2 map: the floor (normal_mat = mat3(1)), the golden monkey, the textured quad as the car."""
    view, lvp, draws, mats = P.demo_scene()
    (_, _, vel), ref = check_pbr(ctx, view, lvp, draws, mats, tile=tile, pcf=pcf, use_shadow=use_shadow)
    assert vel.any()                                   # this demo has a motion buffer
    if not use_shadow:
        assert (ref["prequant"][..., 3][ref["tri_id"] >= 0] == 1.0).all()


@pytest.mark.parametrize("which", ["rough", "metal"])
@pytest.mark.parametrize("name", ["windings", "near", "coincident", "outside"])
def test_scene(ctx, name, which):
    """test_canvas_rt_ref's edge scenes under a rough dielectric (the last mip) and a smooth metal, the normals turned
    by caller-supplied normal matrices so that every cube face is chosen."""
    view, lvp, draws, mats = P.edge_scene(name, which)
    check_pbr(ctx, view, lvp, draws, mats)


def test_without_an_ibl_and_with_one_replaced(ctx):
    """No IBL (the monkey's blue byte 0: channels at exactly 0 where the light does not reach); then an IBL of other
    sizes set after a frame with the first: the second frame uses the new levels."""
    view, lvp, draws, mats = P.demo_scene(monkey_color=(240, 195, 0, 255))
    (color, _, _), ref = check_pbr(ctx, view, lvp, draws, mats, ibl=None)
    assert ((color[..., :3] == 0) & (ref["tri_id"] >= 0)[..., None]).sum() > 100
    other = P.make_ibl(3, 5, 6, 3)                      # irradiance 5^2, specular 6, 3, 1
    (first, _, _), _ = check_pbr(ctx, view, lvp, draws, mats, ibl=IBL)
    (second, _, _), _ = check_pbr(ctx, view, lvp, draws, mats, ibl=other)
    assert (first != second).any() and (first != color).any()


@pytest.mark.parametrize("consts", [dict(exposure=0.9, min_roughness=0.1, direct_intensity=5.0), P.SATURATING], ids=["other", "saturating"])
def test_other_constants(ctx, consts):
    view, lvp, draws, mats = P.demo_scene()
    (color, _, _), _ = check_pbr(ctx, view, lvp, draws, mats, consts=P.demo_consts(**consts))
    if consts is P.SATURATING:
        assert (color[..., :3] == 255).sum() > 1000


def test_frame_size_sequence_alternating_shadings(ctx):
    """1x1, 33x31, 160x120 and 33x31 again through one context with shading 2, 0, 1, 2: the hard and the soft frames
    still equal their own references bit for bit."""
    for ((w, h), sm), shading in zip([((1, 1), 8), ((33, 31), 50), ((160, 120), 96), ((33, 31), 8)], (2, 0, 1, 2)):
        view, proj = R.camera(w, h)
        _, lvp, draws, mats = P.demo_scene()
        draws = [R._rt_draw(d.mesh, d.model, view, proj, color=d.base_color, tex=d.albedo_tex) for d in draws]
        if shading == 2:
            check_pbr(ctx, view, lvp, draws, mats, w=w, h=h, sm=sm)
        elif shading == 1:
            k = S.demo_pcss(**S.WIDE)
            ref_sm = R.ref_shadow(sm, lvp, draws)
            ctx.rt_render_shadow(sm, lvp, draws)
            frame = S.soft_frame(view, lvp, w, h)
            ctx.rt_set_pcss(k)
            try:
                T.check_camera(ctx, frame, draws, S.ref_render_soft(frame, draws, ref_sm, k))
            finally:
                ctx.rt_set_pcss(None)
        else:
            T.check_both(ctx, view, lvp, draws, w=w, h=h, sm=sm)


def test_ibl_samples_known_answers(ctx):
    irr, spec, col = P.face_colour_ibl()
    ctx.rt_set_ibl(irr, spec)
    cases = P.ibl_known_cases()
    a, b = ctx.rt_ibl_samples([c[1] for c in cases], [c[2] for c in cases])
    ra, rb, _ = P.ref_ibl_samples((irr, spec), [c[1] for c in cases], [c[2] for c in cases])
    for i, (name, _, _, face, _, _) in enumerate(cases):
        want = np.zeros(3, F) if face is None else col[face]
        assert np.array_equal(a[i], want) and np.array_equal(b[i], want), (name, a[i], b[i])
    assert np.array_equal(_bits(a), _bits(ra)) and np.array_equal(_bits(b), _bits(rb))
    ctx.rt_set_ibl(None)


@pytest.mark.parametrize("ibl", [IBL, P.make_ibl(5, 1, 1, 1), P.make_ibl(9, 3, 5, 6)], ids=["4-8x4", "1-1x1", "3-5x6"])
def test_ibl_samples_random(ctx, ibl):
    """4,096 seeded directions of every length with lods from below 0 to above the last mip: bit-exact."""
    d, lod = P.random_directions(mips=len(ibl[1]))
    ctx.rt_set_ibl(*ibl)
    a, b = ctx.rt_ibl_samples(d, lod)
    ctx.rt_set_ibl(None)
    ra, rb, _ = P.ref_ibl_samples(ibl, d, lod)
    for got, ref, what in ((a, ra, "irradiance"), (b, rb, "specular")):
        bad = np.argwhere((_bits(got) != _bits(ref)).any(-1))
        assert bad.size == 0, f"{what}: {len(bad)} of {len(ref)} samples differ, first {bad[:4].ravel().tolist()}"


def test_ibl_samples_zero_and_nan_directions(ctx):
    """test_canvas_rt_pbr_ref.edge_directions: equal to the restatement's bits where it gives numbers, NaN where it gives NaN."""
    d, lod = P.edge_directions()
    ctx.rt_set_ibl(*IBL)
    a, b = ctx.rt_ibl_samples(d, lod)
    ctx.rt_set_ibl(None)
    ra, rb, _ = P.ref_ibl_samples(IBL, d, lod)
    assert np.array_equal(P.canonical_bits(a), P.canonical_bits(ra)), (a, ra)
    assert np.array_equal(P.canonical_bits(b), P.canonical_bits(rb)), (b, rb)


def test_end_to_end_on_the_device(ctx, oracle_mod):
    """PASS0, the PBR PASS1, then shs_rt_device_targets into shs_canvas_motion_blur(SHS_CANVAS_DEVICE): equal, byte for
    byte, to the oracle's pass over the planes the device resolved (themselves equal to the restatement's but for
    bytes the parity rule allows)."""
    import torch
    from shs_gpu import _abi
    view, lvp, draws, mats = P.demo_scene()
    _, proj = R.camera()
    ctx._on_torch_stream()
    (color, depth, vel), ref = check_pbr(ctx, view, lvp, draws, mats)
    ctx.rt_set_ibl(*IBL)
    ctx.rt_render_pbr(P.pbr_frame(view, lvp), draws, mats)
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
    ctx.rt_set_ibl(None)
    got = dst.cpu().numpy()
    want = oracle_mod.canvas_motion_blur(color, ref["depth"], ref["velocity"], view, proj, view, proj)
    bad = np.argwhere((got != want).any(-1))
    assert bad.size == 0, f"{len(bad)} pixels differ, first {bad[:4].tolist()}"
    assert (got != color).any()


def test_rejections():
    import shs_gpu
    view, lvp, draws, mats = P.edge_scene("windings", "rough")
    nan, inf = float("nan"), float("inf")
    with shs_gpu.Context(0) as c:
        frame = P.pbr_frame(view, lvp)

        def rejected(call, what):
            with pytest.raises(shs_gpu.ShsError) as e:
                call()
            assert e.value.code == -1, what

        rejected(lambda: c.rt_render_pbr(frame, draws, mats), "SHS_RT_USE_SHADOW before any shadow pass")
        c.rt_render_shadow(SM, lvp, draws)
        for shading in (0, 1, 3, -1):
            rejected(lambda: c.rt_render_pbr(dataclasses.replace(frame, shading=shading), draws, mats), f"shading {shading}")
        rejected(lambda: c.rt_render_pbr(frame, draws, mats[:-1]), "fewer materials than draws")
        rejected(lambda: c.rt_render_pbr(frame, draws, mats + mats[:1]), "more materials than draws")
        rejected(lambda: c.rt_render_pbr(frame, [dataclasses.replace(draws[0], mesh=999)] + draws[1:], mats), "unknown mesh")
        rejected(lambda: c.rt_render_pbr(frame, [dataclasses.replace(draws[0], albedo_tex=77)] + draws[1:], mats), "unknown texture")
        rejected(lambda: c.rt_render_pbr(dataclasses.replace(frame, width=0), draws, mats), "width 0")
        with pytest.raises(shs_gpu.ShsError) as e:      # shs_rt_render still has no shading 2
            c.rt_render(frame, draws)
        assert e.value.code == -1 and "shading" in str(e.value)
        for bad in (dict(exposure=nan), dict(min_roughness=inf), dict(direct_intensity=-inf)):
            rejected(lambda: c.rt_set_pbr(P.demo_consts(**bad)), bad)
        irr, spec = IBL
        c.rt_set_ibl(irr, spec)
        rejected(lambda: c.rt_set_ibl(irr, []), "mip_count 0")
        rejected(lambda: c.rt_set_ibl(irr, spec + [spec[-1]] * 13), "mip_count 17")
        rejected(lambda: c.rt_set_ibl(np.zeros((6, 0, 0, 3), F), spec), "irr_size 0")
        rejected(lambda: c.rt_set_ibl(irr, [np.zeros((6, 0, 0, 3), F)]), "spec_base 0")
        # the rejected constants and levels were not kept, and the context still renders: the frame is the demo
        # constants' under the IBL set before the rejections
        ref_sm = R.ref_shadow(SM, lvp, draws)
        ref = P.ref_render_pbr(frame, draws, mats, ref_sm, IBL)
        c.rt_render_pbr(frame, draws, mats)
        color, depth, _ = c.rt_resolve()
        helpers.assert_depth_bitexact(depth, ref["depth"])
        pq = c.rt_resolve_prequant()
        helpers.assert_color_parity(color, ref["color"], pq, ref["prequant"])
        assert np.abs(pq[..., :3] - ref["prequant"][..., :3]).max() <= helpers.TOL * 255.0
        assert (c.rt_resolve_ids() >= 0).sum() > 1000
