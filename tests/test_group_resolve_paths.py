"""Tile groups, the resolve loop's two bodies (raster_group, shs_legacy.hip).  A wave of a single-draw
frame whose covered lanes' keys all carry a staging slot reads the winners' records from their LDS copies,
takes the frame's draw -- uniforms and shading model -- from scalars loaded at draws[frame], and branches
on the model once per wave; every other wave (frames of several draws, multi-pass groups, a ghost fragment
among the winners) takes shade_stored_winner whole.  Both store through the tile's scalar plane bases with
32-bit offsets.  raster_tile keeps the helpers it had, so the context with a work item per tile is the
reference for every bit; one context per case also goes against the CPU oracle.

Frames of at most 128x48 px, scan mode forced, rendered three ways -- the default context (groups +
spans), set_group_spans(False), set_tile_groups(False) -- every enabled plane compared bit for bit.

The store has one path at every frame size (a tile-relative offset never needs more than 32 bits), so there
is no large-frame path left to cover."""
import numpy as np
import pytest

from test_gpu_parity import _hair_soup, _identity_draw
from test_group_scalar_views import _oracle_frames, _soup_draw, _strip_tris, box_ctx, ctx, tile_ctx  # noqa: F401
from test_group_spans import _check3
from test_stale_clear import _frame
from test_tile_groups import GROUP_H, GROUP_W, _clutter, _mesh_px

gpu = pytest.mark.gpu

FLT_MAX = np.finfo(np.float32).max


def _own_uniforms(d, k):
    """Frame k's camera, light and colour: no two frames of a batch shade alike."""
    d.camera_pos = np.asarray([0.07 * k - 2.0, 1.5 - 0.05 * k, -3.0 - 0.11 * k], np.float32)
    d.light_dir = np.asarray([np.cos(0.37 * k), -0.6 - 0.01 * k, np.sin(0.37 * k)], np.float32)
    d.color = (30 + (k * 37) % 220, 30 + (k * 91) % 220, 30 + (k * 53) % 220, 255)
    return d


@gpu
def test_more_single_draw_frames_than_lds_draws(ctx, box_ctx, tile_ctx, oracle_mod):
    """66 frames x 1 draw at 64x16 (one group each): 66 > LDS_DRAWS (64), so frames 64 and 65 had their
    uniforms fetched per pixel from the device table; now every frame's come from draws[frame] as scalars.
    All four models take turns; each frame has its own mesh, camera, light and colour."""
    W, H = GROUP_W, GROUP_H
    fds = [[_own_uniforms(_soup_draw(W, H, 24, 500 + k, k % 4, kind="small"), k)] for k in range(66)]
    _check3(ctx, box_ctx, tile_ctx, _frame(W, H, present=True, prequant=True), fds, "66 x 1 draw")
    assert ctx.stats()["covered_pixels"] > 66 * 50
    a, b = ctx.resolve_frame(63)[0], ctx.resolve_frame(65)[0]
    assert not np.array_equal(a, b), "the frames do not differ"
    _oracle_frames(ctx, oracle_mod, W, H, fds, frames={0, 63, 64, 65})


@gpu
def test_one_model_per_single_draw_frame(ctx, box_ctx, tile_ctx, oracle_mod):
    """Four single-draw frames, one per shading model (Flat, Gouraud, Phong, Blinn-Phong), each one group
    of clutter: a workgroup resolves one frame's group after another's, so the scalar model and uniforms
    must be the group's own frame's.  Then the models in reverse order on the same contexts."""
    W, H = 128, 48
    fds = [[_own_uniforms(_identity_draw(_clutter(W, H, GROUP_W * (k % 2), GROUP_H * (k // 2), 40, 510 + k), k), k)] for k in range(4)]
    frame = _frame(W, H, present=True, prequant=True)
    _check3(ctx, box_ctx, tile_ctx, frame, fds, "models 0..3")
    assert ctx.stats()["covered_pixels"] > 4 * 100
    _oracle_frames(ctx, oracle_mod, W, H, fds)
    rev = [[_own_uniforms(_identity_draw(d[0].mesh, 3 - k), k + 7)] for k, d in enumerate(fds)]
    _check3(ctx, box_ctx, tile_ctx, frame, rev, "models 3..0")
    _oracle_frames(ctx, oracle_mod, W, H, rev)


@gpu
@pytest.mark.parametrize("n_draws", [2, 3])
def test_several_models_inside_one_group(ctx, box_ctx, tile_ctx, oracle_mod, n_draws):
    """Two or three draws of different models per frame whose triangles overlap inside one group (single
    pass: fewer than 64 candidates): neighbouring lanes of a wave shade with different models and uniforms,
    the per-lane body."""
    W, H = 128, 48
    fds = []
    for f in range(2):
        draws = [_own_uniforms(_identity_draw(_clutter(W, H, GROUP_W, GROUP_H, 18, 520 + 10 * f + i), (i + f + 1) % 4), 3 * f + i)
                 for i in range(n_draws)]
        fds.append(draws)
    _check3(ctx, box_ctx, tile_ctx, _frame(W, H, present=True, prequant=True), fds, f"{n_draws} models in a group")
    assert ctx.stats()["covered_pixels"] > 2 * 100
    col, _ = ctx.resolve_frame(0)
    assert len(np.unique(np.ascontiguousarray(col).view(np.uint32))) > n_draws, "the draws are not all visible"
    _oracle_frames(ctx, oracle_mod, W, H, fds)


@gpu
def test_multi_pass_group_winners_from_hbm(ctx, box_ctx, tile_ctx, oracle_mod):
    """130 triangles in one group of a single-draw frame: more than one staging chunk, so no key carries a
    slot and every wave of the group takes the stored-record body; the frame's other group (40 triangles
    of the same draw) stays single-pass."""
    W, H = 128, 48
    from shs_gpu.scene import Mesh
    fds = []
    for f in range(2):
        a = _clutter(W, H, GROUP_W * f, GROUP_H, 130, 530 + f)
        b = _clutter(W, H, GROUP_W * (1 - f), 2 * GROUP_H, 40, 532 + f)
        mesh = Mesh(np.concatenate([a.positions, b.positions]), np.concatenate([a.normals, b.normals]))
        fds.append([_own_uniforms(_identity_draw(mesh, 3 - f), f)])
    _check3(ctx, box_ctx, tile_ctx, _frame(W, H, present=True, prequant=True), fds, "130 + 40")
    assert ctx.stats()["covered_pixels"] > 2 * 300
    _oracle_frames(ctx, oracle_mod, W, H, fds)


def _ghost_slivers(oracle_mod, W, H, n=48):
    """n hair slivers of test_gpu_parity's soup whose tile-clamp pixels show: the first run of n whose
    oracle render with 80x80 reference tiles differs from its single-tile render."""
    from shs_gpu.scene import Mesh
    pos, nrm = _hair_soup(np.random.default_rng(27), W, H, 2500)
    for c in range(0, len(pos) - n + 1, n):
        d = [_identity_draw(Mesh(pos[c:c + n], nrm[c:c + n]), 3)]
        tiled = oracle_mod.render_legacy(W, H, d, tile=(80, 80), threads=1)[1]
        whole = oracle_mod.render_legacy(W, H, d, tile=(4096, 4096), threads=1)[1]
        if not np.array_equal(tiled.view(np.uint32), whole.view(np.uint32)):
            return pos[c:c + n], nrm[c:c + n]
    raise AssertionError("no run of slivers with visible tile-clamp pixels")


@gpu
def test_ghost_fragments_in_single_pass_groups(ctx, box_ctx, tile_ctx, oracle_mod):
    """48 hair slivers per frame, one draw: every group is single-pass (48 candidates at most), and the
    slivers' tile-clamp pixels arrive as ghost fragments without a slot -- waves with staged and unstaged
    winners side by side, which take the stored-record body whole, next to all-staged waves."""
    from shs_gpu.scene import Mesh
    W, H = 128, 48
    pos, nrm = _ghost_slivers(oracle_mod, W, H)
    fds = [[_own_uniforms(_identity_draw(Mesh(pos, nrm), 3 - k), k)] for k in range(2)]
    _check3(ctx, box_ctx, tile_ctx, _frame(W, H, present=True, prequant=True), fds, "ghosts in single-pass groups")
    st = ctx.stats()
    print("unbounded", st["tri_ghost_unbounded"], "fragments", st["ghost_fragments"], "covered", st["covered_pixels"])
    assert st["ghost_fragments"] > 0, "the scene has no ghost fragments"
    assert st["covered_pixels"] > 0
    _oracle_frames(ctx, oracle_mod, W, H, fds)


@gpu
@pytest.mark.parametrize("planes", [True, False], ids=["present+prequant", "colour+depth"])
def test_edge_tiles_every_plane(ctx, box_ctx, tile_ctx, oracle_mod, planes):
    """72x20, single-draw frames: the last group column is one tile wide with 8 px on the frame, the last
    group row one tile high with 4 rows -- the canvas-row base of a bottom tile is its lowest row that
    exists -- with all four planes and with colour and depth alone."""
    W, H = 72, 20
    big = [[(-8, -8), (W + 8, -8), (-8, H + 8)], [(W + 8, -8), (W + 8, H + 8), (-8, H + 8)]]   # every pixel covered
    fds = [[_own_uniforms(_soup_draw(W, H, 60, 540 + k, 3 - k), k)] for k in range(3)]
    fds.append([_own_uniforms(_identity_draw(_mesh_px(W, H, big + _strip_tris(W, H, 58), np.linspace(-0.5, 0.5, 180).reshape(60, 3)), 2), 3)])
    _check3(ctx, box_ctx, tile_ctx, _frame(W, H, present=planes, prequant=planes), fds, "72x20")
    assert ctx.stats()["covered_pixels"] > W * H
    assert (ctx.resolve_frame(3)[1] < FLT_MAX).all(), "the covering frame has holes"
    _oracle_frames(ctx, oracle_mod, W, H, fds)
