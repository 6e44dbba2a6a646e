"""Tile groups, the group's keys (raster_group, shs_legacy.hip): one row-major array of GY * RTH rows of
GX * RTW keys, addressed by (group row) * 64 + (group x) from the pair loops, the ghost fragments, the
resolve loop's read and reset and the initialisation.  Only the group's busy tiles are resolved and reset, so
a key written into another tile would stay for the workgroup's later items: a sharded frame's pairs and
fragments look their tile up in the busy mask, an unsharded frame's pairs cannot meet an idle tile (setup
marks every tile of a triangle's bin box).

Batches of 2-6 frames of at most 200x48 px, scan mode forced, rendered three ways -- the default context
(groups + spans), set_group_spans(False), set_tile_groups(False) -- every enabled plane compared bit for bit;
one context per case also goes against the CPU oracle, depth exact.

At these sizes the raster's grid has a workgroup per item, so a key left behind meets no later item.  The
last test therefore renders batches of 300 small frames (2,100 items over 1,024 workgroups: every workgroup
takes several groups, with other tiles busy) on the group and the per-tile contexts."""
import numpy as np
import pytest

from helpers import assert_color_parity, assert_depth_bitexact
from test_batch import _owned_mask
from test_gpu_parity import _hair_soup, _identity_draw
from test_group_pairs import _tile_clutter, _wide_tris
from test_group_resolve_paths import _own_uniforms
from test_group_scalar_views import _oracle_frames, _soup_draw, box_ctx, ctx, tile_ctx  # noqa: F401
from test_group_spans import _check3
from test_stale_clear import _frame, _planes
from test_tile_groups import GROUP_H, GROUP_W, _clutter, _cover_draw

gpu = pytest.mark.gpu

FLT_MAX = np.finfo(np.float32).max
RTW, RTH = 32, 8


@gpu
@pytest.mark.parametrize("W,H", [(72, 20), (130, 33)])
def test_edge_groups_have_fewer_columns_and_rows(ctx, box_ctx, tile_ctx, oracle_mod, W, H):
    """72x20: the last group column is one tile wide (8 px on the frame), the last group row one tile high
    (4 rows).  130x33: the last column holds 2 px, the last row one pixel row.  The rows of an edge group
    are still 64 keys apart."""
    fds = [[_own_uniforms(_soup_draw(W, H, 90, 160 + k, 3 - k), k)] for k in range(3)]
    _check3(ctx, box_ctx, tile_ctx, _frame(W, H, present=True, prequant=True), fds, f"{W}x{H}")
    assert ctx.stats()["covered_pixels"] > W * H
    _oracle_frames(ctx, oracle_mod, W, H, fds)


def _sliver_frame(W, H, seeds, n):
    from shs_gpu.scene import Mesh
    soups = [_hair_soup(np.random.default_rng(s), W, H, n) for s in seeds]
    return [_identity_draw(Mesh(np.concatenate([p for p, _ in soups]), np.concatenate([q for _, q in soups])), 3)]


def _ghost_tiles(oracle_mod, W, H, draws, tile):
    """{group (column, row): the tiles of it -- ty * 2 + tx -- with a visible tile-clamp pixel}: where the
    oracle's render with the reference tiles differs from its single-tile render."""
    tiled = oracle_mod.render_legacy(W, H, draws, tile=tile, threads=8)[1]
    whole = oracle_mod.render_legacy(W, H, draws, tile=(4096, 4096), threads=8)[1]
    ys, xs = np.nonzero(tiled.view(np.uint32) != whole.view(np.uint32))
    out = {}
    for y, x in zip(ys.tolist(), xs.tolist()):
        out.setdefault((x // GROUP_W, y // GROUP_H), set()).add(((y % GROUP_H) // RTH) * 2 + (x % GROUP_W) // RTW)
    return out


@gpu
@pytest.mark.parametrize("tile,seeds,n", [((80, 80), (102, 105, 115), 3000), ((24, 24), (28, 1028), 1500), ((7, 7), (28, 1028), 1500)],
                         ids=["80", "24", "7"])
def test_sliver_soup_ghost_fragments_in_every_tile_of_a_group(ctx, box_ctx, tile_ctx, oracle_mod, tile, seeds, n):
    """192x48 hair slivers, a soup per frame, under reference tiles of 80 (job seams at x = 80 inside the group
    [64, 127] and at x = 160, between the tiles of the group [128, 191]), 24 and 7: the tile clamp's pixels
    outside the slivers' boxes arrive as ghost fragments.  Those the oracle shows (its render with the
    reference tiles against its single-tile render) lie, over the batch's frames, in all four tiles of one
    group position at least."""
    W, H = 192, 48
    fds = [_sliver_frame(W, H, (s,), n) for s in seeds]
    ghosts = {}
    for d in fds:
        for g, t in _ghost_tiles(oracle_mod, W, H, d, tile).items():
            ghosts.setdefault(g, set()).update(t)
    print("tiles with visible tile-clamp pixels, per group:", {g: sorted(t) for g, t in sorted(ghosts.items())})
    assert any(len(t) == 4 for t in ghosts.values()), "no group has tile-clamp pixels in all four tiles"
    if tile == (80, 80):
        assert any(g[0] == 1 for g in ghosts), "nothing at the x = 80 seam"
    frame = _frame(W, H, present=True, prequant=True, ref_tile=tile)
    _check3(ctx, box_ctx, tile_ctx, frame, fds, f"slivers, reference tiles {tile}")
    st = ctx.stats()
    print("unbounded", st["tri_ghost_unbounded"], "fragments", st["ghost_fragments"])
    assert st["ghost_fragments"] > 0
    _oracle_frames(ctx, oracle_mod, W, H, fds, ref_tile=tile)


@gpu
def test_keys_kept_across_chunks_and_scan_rounds(ctx, box_ctx, tile_ctx, oracle_mod):
    """130 candidates in one group (three staging chunks: its keys live across their pair passes) among 1,100
    triangles per frame (two scan rounds); the frames swap roles between the batches."""
    W, H = 128, 48
    big = [_soup_draw(W, H, 1000, 181, 3), _soup_draw(W, H, 100, 184, 1, (0, 90, 255, 255))]
    many = [_identity_draw(_clutter(W, H, GROUP_W, GROUP_H, 130, 182), 3, (255, 0, 0, 255)),
            _soup_draw(W, H, 970, 183, 2, (0, 255, 0, 255), kind="off")]
    frame = _frame(W, H, present=True, prequant=True)
    _check3(ctx, box_ctx, tile_ctx, frame, [big, many], "1100 | 130")
    _check3(ctx, box_ctx, tile_ctx, frame, [many, big], "130 | 1100")
    _oracle_frames(ctx, oracle_mod, W, H, [many, big])


def _raw(c, W, H, k):
    return _planes(c, _frame(W, H, present=True, prequant=True), k)


@gpu
@pytest.mark.parametrize("rank,count", [(0, 2), (1, 2), (0, 3), (1, 3), (2, 3)])
def test_sharded_boxes_cross_other_shards_tiles(ctx, box_ctx, tile_ctx, oracle_mod, rank, count):
    """Triangles 50-64 px wide: every box crosses 32x32 tiles of the other shards inside its groups.  The
    owned tiles equal the oracle; the others keep, in every plane, what the batch before -- a fresh context's
    first, which clears in full and draws into every tile -- left there."""
    W, H = 200, 48
    fds = [[_own_uniforms(_identity_draw(_wide_tris(W, H, 40, 190 + k), 3 - k), k)] for k in range(2)]
    cover = [[_cover_draw(W, H)], [_cover_draw(W, H)]]
    _check3(ctx, box_ctx, tile_ctx, _frame(W, H, present=True, prequant=True), cover, "every tile busy")
    before = [_raw(ctx, W, H, k) for k in range(2)]
    sharded = _frame(W, H, shard_rank=rank, shard_count=count, present=True, prequant=True)
    _check3(ctx, box_ctx, tile_ctx, sharded, fds, f"shard {rank}/{count}", raw=True)
    own = _owned_mask(sharded)
    other = {"color": ~own[::-1], "depth": ~own, "present": ~own, "prequant": ~own[::-1][..., None]}
    for k in range(2):
        after = _raw(ctx, W, H, k)
        for plane, m in other.items():
            assert np.array_equal(np.where(m, after[plane], 0), np.where(m, before[k][plane], 0)), \
                f"frame {k}: {plane}: another shard's pixels changed"
        rc, rd, rpq = oracle_mod.render_legacy(W, H, fds[k], tile=sharded.ref_tile, threads=8, prequant=True)
        gc, gd = ctx.resolve_frame(k)
        gpq = ctx.resolve_prequant(k)
        assert_depth_bitexact(np.where(own, gd, 0.0), np.where(own, rd, 0.0))
        mc = own[::-1][..., None]
        assert_color_parity(np.where(mc, gc, 0), np.where(mc, rc, 0), np.where(mc, gpq, 0), np.where(mc, rpq, 0))
        assert int((own & (rd < FLT_MAX)).sum()) > 100, "the shard draws next to nothing"
    _check3(ctx, box_ctx, tile_ctx, _frame(W, H, present=True, prequant=True), fds, "unsharded after the shard")


@gpu
def test_second_batch_draws_nothing_in_the_firsts_groups(ctx, box_ctx, tile_ctx, oracle_mod):
    """Two batches on the same contexts: the first fills the groups at (0, 0) and (64, 32), the second draws in
    the other groups alone.  The first's groups must come out clear, the second's as the oracle has them."""
    W, H = 192, 48
    frame = _frame(W, H, present=True, prequant=True)
    first = [[_own_uniforms(_identity_draw(_clutter(W, H, 0, 0, 50, 200 + k), 3), k),
              _own_uniforms(_identity_draw(_clutter(W, H, GROUP_W, 2 * GROUP_H, 50, 210 + k), 2), k + 3)] for k in range(3)]
    second = [[_own_uniforms(_identity_draw(_clutter(W, H, GROUP_W, 0, 50, 220 + k), 3), k),
               _own_uniforms(_identity_draw(_clutter(W, H, 2 * GROUP_W, GROUP_H, 50, 230 + k), 1), k + 3)] for k in range(3)]
    _check3(ctx, box_ctx, tile_ctx, frame, first, "first batch")
    assert ctx.stats()["covered_pixels"] > 3 * 400
    _check3(ctx, box_ctx, tile_ctx, frame, second, "second batch")
    clear = np.float32(FLT_MAX).view(np.uint32)
    for k in range(3):
        z = _planes(ctx, frame, k)["depth"]
        assert (z[:GROUP_H, :GROUP_W] == clear).all() and (z[2 * GROUP_H:, GROUP_W:2 * GROUP_W] == clear).all(), \
            f"frame {k}: the first batch's groups are not clear"
        assert not (z[:GROUP_H, GROUP_W:2 * GROUP_W] == clear).all()
    _oracle_frames(ctx, oracle_mod, W, H, second)


@gpu
@pytest.mark.parametrize("count", [1, 2], ids=["unsharded", "two shards"])
def test_workgroups_that_take_several_groups(ctx, tile_ctx, count):
    """300 frames of 96x48 (six groups and a clear strip each: 2,100 items for at most 1,024 workgroups), four
    scenes by turns whose groups have different tiles busy -- and, with two shards, owned: the 32x32 tiles
    alternate along a row and between the rows, so a group's left tiles are this shard's at y < 32 and the
    other's below.  A workgroup's next group starts from the keys its last one left, so every key written
    must have been reset.  Groups against a work item per tile, every frame, every plane, other shards'
    pixels included."""
    from shs_gpu.scene import Mesh
    W, H, n = 96, 48, 300
    scenes = []
    for s in range(4):
        parts = [_wide_tris(W, H, 4, 240 + s)]   # across the tile columns: pairs in tiles of the other shard
        for cy in range(3):
            t = (s + cy) % 4      # one tile of the group at x = 0 (another per scene and group row) ...
            parts.append(_tile_clutter(W, H, (t % 2) * RTW, cy * GROUP_H + (t // 2) * RTH, 10, 250 + 10 * s + cy))
            # ... and one of the two of the group at x = 64
            parts.append(_tile_clutter(W, H, GROUP_W, cy * GROUP_H + ((s + cy) % 2) * RTH, 10, 255 + 10 * s + cy))
        mesh = Mesh(np.concatenate([m.positions for m in parts]), np.concatenate([m.normals for m in parts]))
        scenes.append([_identity_draw(mesh, 3 - s, (40 + 50 * s, 200 - 40 * s, 90, 255))])
    fds = [scenes[(k + k // 7) % 4] for k in range(n)]
    cover = [[_cover_draw(W, H)]] * n
    frame = _frame(W, H, shard_rank=0, shard_count=count)
    for c in (ctx, tile_ctx):
        c.render_batch(_frame(W, H), cover)
        c.render_batch(frame, fds)
    assert ctx.stats()["covered_pixels"] > n * 30
    view = _frame(W, H)   # raw planes
    bad = [k for k in range(n)
           if any(not np.array_equal(a, b) for a, b in zip(_planes(ctx, view, k).values(), _planes(tile_ctx, view, k).values()))]
    assert not bad, f"{len(bad)} frames differ from the per-tile render, the first: {bad[:8]}"
