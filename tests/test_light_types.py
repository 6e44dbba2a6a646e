"""GPU tests of SHS_PROGRAM_FORWARD_PLUS_TYPED: spot, rect-area and tube-area lights shaded per pixel.

Reference: the frozen oracle's rasteriser, varyings and list selection with every listed light evaluated by
the C restatement of the four ILightModel::sample functions (tests/light_types_ref, test_light_types_ref.py's
typed_reference).  Lists and depth: exact.  Shaded HDR: within the project's 1e-5 (helpers.assert_float_close),
no pixel left out -- the GPU and the reference do the same IEEE operations on the same varyings; the branch
that hangs on a pow result (attenuation_cutoff) is only used with attenuation_power == 1."""
import numpy as np
import pytest

from helpers import assert_depth_bitexact, assert_float_close
from test_light_types_ref import typed_reference

pytestmark = pytest.mark.gpu

W, H = 200, 130      # edge tiles in the 32x32 bin grid, the 32x8 raster grid and the 16-px light grid


def _scene(mode=1, tile=16, maxp=128, n_draws=4):
    from shs_gpu import scene_lib
    frame, draws, _, cull = scene_lib.c4_scene(W, H, n_objects=40, tris_per_object=100, n_draws=n_draws, n_lights=1, mode=mode,
                                               tile_size=tile, max_per_tile=maxp)
    return frame, draws, cull


def _with_program(draws, program):
    return [type(d)(**{**d.__dict__, "program": program}) for d in draws]


def _mixed_props(n):
    from shs_gpu import scene_lib
    return np.ascontiguousarray(scene_lib.c4_lights_typed(n))


def _typed_frame(ctx, oracle_mod, monkeypatch, frame, draws, cull, props, check_ref=True):
    """Typed upload -> depth prepass -> light cull -> the draws on the GPU; lists exact against the oracle's
    cull of the packed records; HDR and depth against the typed reference.  -> (hdr, depth, list counts)."""
    recs = ctx.upload_lights_typed(props)
    ctx.render_pbr_forward(frame, _with_program(draws, 2))
    _, depth, _ = ctx.resolve_lib()
    ctx.light_cull(cull)
    gc, gi, _ = ctx.resolve_light_lists()
    rc, ri, _ = oracle_mod.light_cull(cull, recs, depth)
    assert np.array_equal(gc, rc), f"{int((gc != rc).sum())} list counts differ"
    for l in np.nonzero(rc)[0]:
        assert np.array_equal(gi[l, :rc[l]], ri[l, :rc[l]]), f"list {l} differs"
    ctx.render_pbr_forward(frame, draws)
    gh, gd, _ = ctx.resolve_lib()
    if check_ref:
        rh, rd, _, _ = typed_reference(monkeypatch, oracle_mod, frame, draws, recs, props, cull, (rc, ri))
        assert_depth_bitexact(gd, rd)
        assert_float_close(gh, rh, what="typed forward+ hdr")
    return gh, gd, gc


def test_point_set_typed_equals_program_5_bitwise(gpu_ctx):
    """A point-only set uploaded typed and drawn with program 6 == program 5 after the old upload: lists,
    depth and HDR bit for bit."""
    from shs_gpu import scene_lib
    frame, draws, cull = _scene()
    props = scene_lib.c4_lights_typed(64)
    props["type"] = 1
    gpu_ctx.upload_lights(scene_lib.c4_lights(64))
    gpu_ctx.light_cull(cull)
    c5, i5, _ = gpu_ctx.resolve_light_lists()
    gpu_ctx.render_pbr_forward(frame, draws)
    h5, d5, _ = gpu_ctx.resolve_lib()
    recs = gpu_ctx.upload_lights_typed(props)
    assert recs.tobytes() == scene_lib.c4_lights(64).tobytes()
    gpu_ctx.light_cull(cull)
    c6, i6, _ = gpu_ctx.resolve_light_lists()
    gpu_ctx.render_pbr_forward(frame, _with_program(draws, 6))
    h6, d6, _ = gpu_ctx.resolve_lib()
    assert np.array_equal(c5, c6) and c5.max() > 0
    for l in np.nonzero(c5)[0]:
        assert np.array_equal(i5[l, :c5[l]], i6[l, :c5[l]])
    assert_depth_bitexact(d6, d5)
    assert np.array_equal(h6.view(np.uint32), h5.view(np.uint32)), "typed point lights differ from program 5"
    assert (h5[d5 < 1.0][:, :3] > 0.4).any()   # lit beyond the ambient term somewhere
    # program 5 after the typed upload still renders, lit as points
    gpu_ctx.render_pbr_forward(frame, draws)
    h5b, _, _ = gpu_ctx.resolve_lib()
    assert np.array_equal(h5b.view(np.uint32), h5.view(np.uint32))


@pytest.mark.parametrize("mode,tile,maxp", [(1, 16, 128), (2, 16, 128), (3, 32, 16), (1, 8, 4)])
def test_typed_frame_vs_reference(gpu_ctx, oracle_mod, monkeypatch, mode, tile, maxp):
    """48 lights, 12 of each type, through every list mode; (1, 8, 4) saturates lists (every-light fallback)."""
    frame, draws, cull = _scene(mode, tile, maxp)
    props = _mixed_props(48)
    assert all(int((props["type"] == t).sum()) == 12 for t in (1, 2, 3, 4))
    _, _, counts = _typed_frame(gpu_ctx, oracle_mod, monkeypatch, frame, _with_program(draws, 6), cull, props)
    if maxp == 4:
        assert (counts >= 4).any(), "no saturated list: the every-light fallback is not exercised"


def test_typed_frame_differs_from_point_shading(gpu_ctx, oracle_mod, monkeypatch):
    """The same mixed set under program 5 (lit as points) is a different image: the models are in use."""
    frame, draws, cull = _scene()
    props = _mixed_props(48)
    h6, _, _ = _typed_frame(gpu_ctx, oracle_mod, monkeypatch, frame, _with_program(draws, 6), cull, props, check_ref=False)
    gpu_ctx.render_pbr_forward(frame, draws)
    h5, _, _ = gpu_ctx.resolve_lib()
    assert np.abs(h6 - h5).max() > 0.05


def test_more_lights_than_the_lds_table(gpu_ctx, oracle_mod, monkeypatch):
    """300 mixed lights (> LIB_LDS_LIGHTS = 256): bounding spheres and records come from global memory."""
    frame, draws, cull = _scene()
    _typed_frame(gpu_ctx, oracle_mod, monkeypatch, frame, _with_program(draws, 6), cull, _mixed_props(300))


def _edge_set():
    """The CPU known-answer lights over a floor quad (y = 0, x in [-8, 8], z in [0, 16]), their edges on it."""
    from shs_gpu.lib_path import light_props
    p = light_props(12)
    t = p["type"]
    t[:] = (2, 2, 3, 3, 3, 4, 4, 1, 1, 2, 4, 3)
    p["position_ws"] = [(-5, 3, 3), (-5, 3, 9), (0, 1, 4), (4, 1.5, 3), (5, 2, 12), (0, 1, 9), (-4, 1, 13), (5, 2, 8),
                        (-1, 2, 14), (2, 3, 6), (3, 1, 14), (-6, 2, 6)]
    p["range"] = (8, 8, 5, 4, 3, 3, 3, 3, 4, 6, 4, 5)
    p["color"] = [(1, 0.6, 0.4), (0.4, 1, 0.6), (0.5, 0.6, 1), (1, 1, 0.5), (0.9, 0.4, 0.9), (0.4, 0.9, 0.9), (1, 0.5, 0.5),
                  (0.6, 1, 0.4), (0.8, 0.8, 1), (1, 0.8, 0.6), (0.7, 1, 0.7), (1, 0.7, 0.9)]
    p["intensity"] = 1.5
    p["direction_ws"][1] = (0, 0, 0)                       # zero direction: (0, -1, 0); cone edge on the floor
    p["direction_ws"][2], p["up_ws"][2] = (1, 0, 0), (0, 1, 0)   # rect facing +x: its plane x = 0 crosses the floor
    p["up_ws"][3], p["rect_half_extents"][3] = (0, 0, 1), (0.01, 0.02)   # facing down, extents below the 0.05 floor
    p["up_ws"][4] = (0, 0, 1)                              # facing down: corners, range edge (range 3 at height 2)
    p["tube_half_length"][5] = 1.5                         # tube ends and its range edge
    p["right_ws"][6], p["tube_half_length"][6] = (0, 0, 2), 0.02   # half length below the 0.1 floor
    p["attenuation_cutoff"][8] = 0.1                       # cutoff with power 1 (point)
    p["attenuation_cutoff"][9] = 0.1                       # ... and under a spot cone
    p["attenuation_model"][10], p["attenuation_power"][10] = 2, 2.5   # InverseSquare, power 2.5 (tube)
    p["attenuation_model"][11], p["attenuation_power"][11], p["up_ws"][11] = 0, 2.5, (0, 0, 1)   # Linear, power 2.5 (rect)
    return np.ascontiguousarray(p)


def test_per_model_edges_on_a_floor_quad(gpu_ctx, oracle_mod, monkeypatch):
    """64x48, one floor quad: cone edge, rect plane, rect corners, tube ends, range edges, the clamps, a zero
    direction, cutoff 0.1 with power 1, InverseSquare and Linear attenuation with power 2.5."""
    from shs_gpu.lib_path import (CULL_NONE, PROGRAM_FORWARD_PLUS_TYPED, LibDraw, LibFrame, LibMesh, LightCull, look_at_lh,
                                  mat_mul, perspective_lh_no)
    w, h, zn, zf = 64, 48, 0.1, 100.0
    q = np.array([(-8, 0, 0), (8, 0, 0), (8, 0, 16), (-8, 0, 0), (8, 0, 16), (-8, 0, 16)], np.float32)
    mesh = LibMesh(positions=q, normals=np.tile(np.array([(0, 1, 0)], np.float32), (6, 1)))
    eye = (np.float32(0.0), np.float32(12.0), np.float32(-4.0))
    view = look_at_lh(eye, (0.0, 0.0, 7.0))
    proj = perspective_lh_no(np.float32(np.deg2rad(60.0)), np.float32(w) / np.float32(h), zn, zf)
    draws = [LibDraw(mesh=mesh, program=PROGRAM_FORWARD_PLUS_TYPED, viewproj=mat_mul(proj, view), camera_pos=eye,
                     base_color=(0.8, 0.7, 0.6), cull_mode=CULL_NONE)]
    frame = LibFrame(w, h, depth_motion=True, zn=zn, zf=zf, bg_gradient=True)
    cull = LightCull(w, h, view, proj, zn=zn, zf=zf, tile_size=16, max_per_tile=128, mode=1)
    props = _edge_set()
    gh, gd, _ = _typed_frame(gpu_ctx, oracle_mod, monkeypatch, frame, draws, cull, props)
    cov = gd < 1.0
    assert cov.sum() > 1000
    lit = gh[cov][:, :3].max(axis=1)
    amb = 0.8 * (0.22 + 0.12)   # base * ambient hemisphere of an up-facing normal
    assert (lit > amb + 0.05).sum() > 200 and (lit < amb + 1e-4).sum() > 50   # lit regions and unlit ones: edges on the quad


def test_mixed_programs_in_one_pass(gpu_ctx, oracle_mod, monkeypatch):
    """One draw each of programs 0, 1, 2 and 6 in one pass (the typed kernel's per-draw dispatch)."""
    frame, draws, cull = _scene(n_draws=4)
    mixed = [type(d)(**{**d.__dict__, "program": prog}) for d, prog in zip(draws, (0, 1, 2, 6))]
    _typed_frame(gpu_ctx, oracle_mod, monkeypatch, frame, mixed, cull, _mixed_props(48))


def _interleaved_mask(rank, count):
    tx = (W + 31) // 32
    ys, xs = np.mgrid[0:H, 0:W]
    return ((ys // 32) * tx + xs // 32) % count == rank


@pytest.mark.parametrize("regions", [False, True])
def test_sharded_ranks_equal_the_unsharded_frame(gpu_ctx, regions):
    """Three ranks (three contexts of device 0), interleaved and region layouts: each rank's owned tiles of
    HDR and depth equal the unsharded frame bit for bit."""
    import shs_gpu
    from test_regions import _check_layout, _mask
    frame, draws, cull = _scene()
    draws = _with_program(draws, 6)
    props = _mixed_props(48)
    gpu_ctx.upload_lights_typed(props)
    gpu_ctx.light_cull(cull)
    gpu_ctx.render_pbr_forward(frame, draws)
    fh, fd, _ = gpu_ctx.resolve_lib()
    count = 3
    ctxs = [shs_gpu.Context(0) for _ in range(count)]
    try:
        seen = np.zeros((H, W), np.int32)
        for r, c in enumerate(ctxs):
            c.set_shard_layout(regions)
            c.upload_lights_typed(props)
            frame.shard_rank, frame.shard_count = r, count
            cull.shard_rank, cull.shard_count = r, count
            c.light_cull(cull)
            c.render_pbr_forward(frame, draws)
            h, d, _ = c.resolve_lib()
            if regions:
                reg = c.shard_regions(count)
                _check_layout(reg, W, H)
                own = _mask(W, H, reg[r])
            else:
                own = _interleaved_mask(r, count)
            seen += own
            assert np.array_equal(h[own].view(np.uint32), fh[own].view(np.uint32)), f"rank {r}: hdr differs"
            assert np.array_equal(d[own].view(np.uint32), fd[own].view(np.uint32)), f"rank {r}: depth differs"
        assert (seen == 1).all()
    finally:
        for c in ctxs:
            c.close()
        frame.shard_rank, frame.shard_count = 0, 1
        cull.shard_rank, cull.shard_count = 0, 1


def test_group_typed_upload_and_gather(gpu_ctx):
    """shs_group, n = 3: upload_lights_typed, sharded cull and pass, gather == the single context's frame."""
    from shs_gpu.group import Group
    frame, draws, cull = _scene()
    draws = _with_program(draws, 6)
    props = _mixed_props(48)
    gpu_ctx.upload_lights_typed(props)
    gpu_ctx.light_cull(cull)
    gpu_ctx.render_pbr_forward(frame, draws)
    fh, fd, _ = gpu_ctx.resolve_lib()
    g = Group([0] * 3)
    try:
        recs = g.upload_lights_typed(props)
        assert len(recs) == 48
        g.light_cull(cull)
        g.render_pbr_forward(frame, draws)
        g.gather(g.root.TARGET_LIB)
        h, d, _ = g.root.resolve_lib()
    finally:
        g.close()
    assert np.array_equal(h.view(np.uint32), fh.view(np.uint32)) and np.array_equal(d.view(np.uint32), fd.view(np.uint32))


def test_errors(gpu_ctx):
    import shs_gpu
    from shs_gpu import scene_lib
    from shs_gpu.lib_path import LIGHT_DTYPE, light_props
    frame, draws, cull = _scene()
    typed = _with_program(draws, 6)
    # program 6 after an old-style upload (and its cull)
    gpu_ctx.upload_lights(scene_lib.c4_lights(16))
    gpu_ctx.light_cull(cull)
    with pytest.raises(shs_gpu.ShsError):
        gpu_ctx.render_pbr_forward(frame, typed)
    # ... and after a typed upload without a cull over it
    gpu_ctx.upload_lights_typed(_mixed_props(16))
    with pytest.raises(shs_gpu.ShsError):
        gpu_ctx.render_pbr_forward(frame, typed)
    for bad in (0, 5):
        with pytest.raises(shs_gpu.ShsError):
            gpu_ctx.upload_lights_typed(light_props(3, bad))
    rect = light_props(2, 3)
    rect["direction_ws"][1], rect["up_ws"][1] = (0, -1, 0), (0, 2, 0)   # up parallel to forward: no basis
    with pytest.raises(shs_gpu.ShsError, match="parallel"):
        gpu_ctx.upload_lights_typed(rect)
    # the C call itself rejects the types too (the Python mirror packs first)
    import ctypes
    from shs_gpu import _abi
    p = light_props(1, 5)
    recs = np.zeros(1, LIGHT_DTYPE)
    rc = gpu_ctx._lib.shs_lights_upload_typed(gpu_ctx._h, recs.ctypes.data_as(ctypes.POINTER(_abi.CullingLightC)),
                                              p.ctypes.data_as(ctypes.POINTER(_abi.LightPropsC)), 1)
    assert rc == _abi.SHS_ERR_INVALID and b"type" in gpu_ctx._lib.shs_last_error(gpu_ctx._h)
    # a failed upload leaves the context usable: a good set, culled, renders
    gpu_ctx.upload_lights_typed(_mixed_props(16))
    gpu_ctx.light_cull(cull)
    gpu_ctx.render_pbr_forward(frame, typed)
    gpu_ctx.resolve_lib()
