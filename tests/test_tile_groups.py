"""Tile groups (SHS_OPT_LEGACY_TILE_GROUPS): a scan-mode legacy batch deals its busy 32x8 raster tiles to
the persistent raster as 2x2 groups (64x16 px) that share one box scan and one staging of the records.

One context (option on, the default) and one with the option at 0 render the same batches, scan mode
forced; every frame of every batch is compared bit for bit -- colour, depth, and the present / prequant
planes where enabled.  One case per size also goes against the CPU oracle (as a frame of a two-frame
batch: a single frame keeps a work item per tile).  Sizes: 1x1, 33x9 (one
partial group), 64x16 (exactly one group), 65x17 and 96x24 (odd group columns / rows: groups of one
column or one row at the edges), 322x181."""
import numpy as np
import pytest

from helpers import FLT_MAX, assert_color_parity, assert_depth_bitexact
from test_gpu_parity import _identity_draw, _ndc_soup
from test_stale_clear import _check, _frame, _hair_sets, _sets

pytestmark = pytest.mark.gpu

SIZES = [(1, 1), (33, 9), (64, 16), (65, 17), (96, 24), (322, 181)]
GROUP_W, GROUP_H, TILE_W, TILE_H = 64, 16, 32, 8


@pytest.fixture(scope="module")
def ref_ctx():
    """Every busy tile its own work item, as before the option existed."""
    import shs_gpu
    ctx = shs_gpu.Context(0)
    ctx.set_tile_groups(False)
    ctx.set_raster_mode(1)
    yield ctx
    ctx.close()


@pytest.fixture()
def ctx():
    import shs_gpu
    c = shs_gpu.Context(0)
    c.set_raster_mode(1)
    yield c
    c.close()


def _check_oracle(c, oracle_mod, frame, draws):
    """Frame 1 of a batch of two such frames against the CPU oracle: depth and coverage bit-exact, colour
    within the parity helper's truncation-boundary rule."""
    frame.prequant = True
    c.render_batch(frame, [draws, draws])
    stats = c.stats()
    gc, gd = c.resolve_frame(1)
    gpq = c.resolve_prequant(1)
    rc, rd, rpq = oracle_mod.render_legacy(frame.width, frame.height, draws, tile=frame.ref_tile, threads=8, prequant=True)
    assert_depth_bitexact(gd, rd)
    assert_color_parity(gc, rc, gpq, rpq)
    assert stats["covered_pixels"] == 2 * int((rd < FLT_MAX).sum())


def _mesh_px(W, H, tris_px, z):
    """Triangles given in pixel space ([n, 3, 2], flipped to positive screen area) with per-corner z
    ([n, 3]) as an identity-MVP mesh."""
    from shs_gpu.scene import Mesh
    p = np.asarray(tris_px, np.float64).copy()
    a = (p[:, 1, 0] - p[:, 0, 0]) * (p[:, 2, 1] - p[:, 0, 1]) - (p[:, 1, 1] - p[:, 0, 1]) * (p[:, 2, 0] - p[:, 0, 0])
    flip = a < 0
    p[flip, 1], p[flip, 2] = p[flip, 2].copy(), p[flip, 1].copy()
    x = p[..., 0] / (0.5 * (W - 1)) - 1.0
    y = 1.0 - p[..., 1] / (0.5 * (H - 1))
    pos = np.stack([x, y, np.asarray(z, np.float64)], axis=2).reshape(-1, 9).astype(np.float32)
    nrm = np.random.default_rng(5).normal(size=pos.shape).astype(np.float32)
    return Mesh(pos, nrm)


def _cover_draw(W, H):
    """Two large triangles over the whole frame: every tile busy (and stale afterwards)."""
    tris = [[(-8, -8), (W + 8, -8), (-8, H + 8)], [(W + 8, -8), (W + 8, H + 8), (-8, H + 8)]]
    return _identity_draw(_mesh_px(W, H, tris, np.full((2, 3), 0.5)), 1)


@pytest.mark.parametrize("W,H", SIZES)
def test_moved_object_then_empty_batch(ctx, ref_ctx, W, H):
    """Multi-frame batches A -> B (the object moved) -> no draws -> A, all four planes enabled: the groups
    change occupancy between batches and workspace slots."""
    n = 3
    A, B = _sets(n, W, H)
    frame = _frame(W, H, present=True, prequant=True)
    _check(ctx, ref_ctx, frame, A, "A")
    _check(ctx, ref_ctx, frame, B, "B")
    _check(ctx, ref_ctx, frame, [[] for _ in range(n)], "empty")
    _check(ctx, ref_ctx, frame, A, "A again")


@pytest.mark.parametrize("W,H", SIZES)
def test_oracle_parity(ctx, oracle_mod, W, H):
    """The default (groups) against the CPU oracle: a Blinn-Phong Suzanne pose at every size."""
    from shs_gpu import scene
    frame, draws = scene.monkey_scene(W, H, 3, yaw=17.0, pitch=-9.0, rotation=23.0)
    _check_oracle(ctx, oracle_mod, frame, draws)


@pytest.mark.parametrize("tile", [0, 1, 2, 3])
@pytest.mark.parametrize("W,H", [(64, 16), (65, 17), (96, 24), (322, 181)])
def test_one_triangle_inside_one_tile(ctx, ref_ctx, oracle_mod, W, H, tile):
    """One busy tile in its group, the other three untouched -- then the same after a batch that drew
    into every tile, so the three idle tiles are cleared by the stale clears while the group runs."""
    gx0 = GROUP_W if W > 2 * GROUP_W else 0
    gy0 = GROUP_H if H > 2 * GROUP_H else 0
    x0, y0 = gx0 + (tile % 2) * TILE_W + 3.2, gy0 + (tile // 2) * TILE_H + 1.1
    tri = _identity_draw(_mesh_px(W, H, [[(x0, y0), (x0 + 22.5, y0 + 0.7), (x0 + 4.0, y0 + 5.6)]], [[0.1, 0.3, -0.2]]), 3)
    frame = _frame(W, H, present=True, prequant=True)
    _check(ctx, ref_ctx, frame, [[tri], [tri]], "one triangle")
    assert ctx.stats()["covered_pixels"] > 20
    _check(ctx, ref_ctx, frame, [[_cover_draw(W, H)], [_cover_draw(W, H)]], "every tile busy")
    _check(ctx, ref_ctx, frame, [[tri], [tri]], "one triangle over dirty planes")
    if tile == 3:
        _check_oracle(ctx, oracle_mod, _frame(W, H), [tri])


def _clutter(W, H, gx0, gy0, n, seed):
    """n small triangles inside the 64x16 region at (gx0, gy0), z quantised to a few values (exact ties)."""
    rng = np.random.default_rng(seed)
    c = rng.uniform([gx0 + 1, gy0 + 1], [gx0 + GROUP_W - 1, gy0 + GROUP_H - 1], size=(n, 1, 2))
    p = np.clip(c + rng.uniform(-7, 7, size=(n, 3, 2)), [gx0 + 0.2, gy0 + 0.2], [gx0 + GROUP_W - 0.2, gy0 + GROUP_H - 0.2])
    z = np.repeat(rng.choice([0.25, 0.5, -0.0, 0.0], size=(n, 1)), 3, axis=1)
    return _mesh_px(W, H, p, z)


@pytest.mark.parametrize("W,H", [(64, 16), (96, 24), (322, 181)])
def test_group_staged_in_several_chunks(ctx, ref_ctx, oracle_mod, W, H):
    """200 small triangles inside one group, all four tiles busy: more candidates than one staging pass
    holds, so every tile's keys live across the passes and the winners are fetched by index."""
    gx0 = GROUP_W if W > 2 * GROUP_W else 0
    gy0 = GROUP_H if H > 2 * GROUP_H else 0
    m = _clutter(W, H, gx0, gy0, 200, 21)
    draws = [_identity_draw(m, 3, (255, 0, 0, 255)), _identity_draw(_clutter(W, H, gx0, gy0, 40, 22), 2, (0, 255, 0, 255))]
    frame = _frame(W, H, present=True, prequant=True)
    _check(ctx, ref_ctx, frame, [draws, draws[::-1]], "clutter")
    _check_oracle(ctx, oracle_mod, _frame(W, H), draws)


def test_more_triangles_than_one_gather_round(ctx, ref_ctx, oracle_mod):
    """A 1,500-triangle scan-mode frame: the box scan takes a second round of 1,024."""
    from shs_gpu.scene import Mesh
    W, H = 322, 181
    fds = []
    for seed in (31, 32):
        pos, nrm = _ndc_soup(np.random.default_rng(seed), W, H, 1500)
        fds.append([_identity_draw(Mesh(pos, nrm), seed % 4)])
    _check(ctx, ref_ctx, _frame(W, H, present=True, prequant=True), fds, "1500 triangles")
    _check_oracle(ctx, oracle_mod, _frame(W, H), fds[0])


@pytest.mark.parametrize("W,H", [(65, 17), (322, 181)])
def test_sliver_soup_ghost_fragments(ctx, ref_ctx, W, H):
    """Sliver soups: some tiles, and some groups, are busy through ghost fragments alone."""
    n = 2
    A, B = _hair_sets(W, H, n, 1500, 500)
    frame = _frame(W, H, present=True, prequant=True)
    _check(ctx, ref_ctx, frame, A, "A")
    if (W, H) == (322, 181):
        assert ctx.stats()["ghost_fragments"] > 0
    _check(ctx, ref_ctx, frame, B, "B")
    _check(ctx, ref_ctx, frame, [[] for _ in range(n)], "empty")
    _check(ctx, ref_ctx, frame, A, "A again")


def test_small_batch_ghost_waves(ctx, ref_ctx, oracle_mod):
    """A small batch's slivers go through the ghost waves (direct marks), not the setup waves' own walk."""
    W, H = 322, 181
    A, _ = _hair_sets(W, H, 2, 600, 900)
    _check(ctx, ref_ctx, _frame(W, H, present=True, prequant=True), A, "two frames")
    _check_oracle(ctx, oracle_mod, _frame(W, H), A[0])


def test_interleaved_shards(ctx, ref_ctx):
    """Two shards on one GPU: a group's two tile columns belong to different shards, so a shard's groups
    have tiles it must not touch."""
    W, H = 322, 181
    A, B = _sets(3, W, H)
    for i, (rank, count, fds) in enumerate([(0, 2, A), (1, 2, A), (1, 2, B), (0, 1, B), (1, 3, A)]):
        _check(ctx, ref_ctx, _frame(W, H, shard_rank=rank, shard_count=count, present=True), fds, f"step {i}: shard {rank}/{count}")


def test_option_toggled_between_batches(ctx, ref_ctx):
    W, H = 322, 181
    A, B = _sets(3, W, H)
    frame = _frame(W, H, present=True)
    for i, (on, fds) in enumerate([(True, A), (False, B), (True, A), (True, B), (False, B), (True, A)]):
        ctx.set_tile_groups(on)
        _check(ctx, ref_ctx, frame, fds, f"step {i}: groups {on}")


def test_ignored_under_the_pipeline(ctx, ref_ctx):
    """SHS_OPT_LEGACY_PIPELINE batches (more than 6 draws in all) keep tile lists; the option stays on."""
    W, H = 322, 181
    A, B = _sets(8, W, H)
    frame = _frame(W, H)
    _check(ctx, ref_ctx, frame, A, "A")
    ctx.set_legacy_pipeline(True)
    _check(ctx, ref_ctx, frame, B, "pipelined B")
    ctx.render_batch(frame, A)          # its raster is still pending when the next batch is enqueued
    _check(ctx, ref_ctx, frame, B, "pipelined B after pending A")
    ctx.set_legacy_pipeline(False)
    _check(ctx, ref_ctx, frame, A, "A after the pipeline")


def test_the_path_is_live(ctx, ref_ctx):
    """The raster timeline's busy-tiles-per-group slot: 1..4 for the default's first items, 0 without groups
    and for a single frame (which keeps a work item per tile)."""
    W, H = 322, 181
    A, _ = _sets(3, W, H)
    frame = _frame(W, H)
    for c in (ctx, ref_ctx):
        c.set_timeline(True)
    try:
        ctx.render_batch(frame, A)
        _, _, r = ctx.debug_timeline()
        tiles = r[:, 12][r[:, 12] != 0]
        assert len(tiles) > 0 and tiles.min() >= 1 and tiles.max() <= 4 and tiles.max() > 1
        ref_ctx.render_batch(frame, A)
        _, _, r0 = ref_ctx.debug_timeline()
        assert (r0[:, 12] == 0).all()
        ctx.render_batch(frame, A[:1])
        _, _, r1 = ctx.debug_timeline()
        assert (r1[:, 12] == 0).all()
        _check(ctx, ref_ctx, frame, A[:1], "a single frame")
    finally:
        ref_ctx.set_timeline(False)
