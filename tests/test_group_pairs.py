"""Tile groups, the pair pass: a busy 2x2 group (64x16 px) lays out the (candidate, pixel) pairs of its
staged candidates' bin boxes clipped to the group rectangle once, and every pair finds its tile -- and
that tile's key array -- from its pixel.  The pair bitmap holds 16,384 pairs; a pass that would exceed it
lays out the leading candidates that fit and continues with the rest.

One context (the default) and one with set_tile_groups(False) (a work item per tile) render the same
batches of >= 2 frames, scan mode forced; every frame and every enabled plane is compared bit for bit.
One case per test also goes against the CPU oracle (depth bit-exact, colour by the parity helper)."""
import numpy as np
import pytest

from test_gpu_parity import _identity_draw
from test_stale_clear import _check, _frame
from test_tile_groups import GROUP_H, GROUP_W, TILE_H, TILE_W, _check_oracle, _mesh_px

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ref_ctx():
    """Every busy tile its own work item."""
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


def _full_frame_tris(W, H, n, seed):
    """n triangles that each cover the whole frame (bin box = the frame: 1,024 pairs in a full group), on
    tilted planes with distinct z so the winner changes across the frame, and a few exact ties (equal
    corners and z: the lower index wins)."""
    rng = np.random.default_rng(seed)
    base = np.array([(-10.0, -10.0), (3.0 * W + 10.0, -10.0), (-10.0, 3.0 * H + 10.0)])
    p = base[None] + rng.uniform(-4.0, 4.0, size=(n, 3, 2))
    z = rng.uniform(0.05, 0.9, size=(n, 3))
    for a, b in ((3, 1), (n - 1, 7), (n // 2, n // 2 - 1)):
        p[a], z[a] = p[b], z[b]
    return _mesh_px(W, H, p, z)


@pytest.mark.parametrize("n", [24, 70])
@pytest.mark.parametrize("W,H", [(64, 16), (65, 17), (96, 24)])
def test_more_pairs_than_the_bitmap_holds(ctx, ref_ctx, oracle_mod, W, H, n):
    """24 x 1,024 pairs in one group: the pass is split inside a staging chunk.  70 triangles: two staging
    chunks, each of them split.  65x17 and 96x24: the edge groups have one tile column or row."""
    a = [_identity_draw(_full_frame_tris(W, H, n, 40 + n), 3)]
    b = [_identity_draw(_full_frame_tris(W, H, n, 41 + n), 1, (30, 220, 90, 255))]
    frame = _frame(W, H, present=True, prequant=True)
    _check(ctx, ref_ctx, frame, [a, b], f"{n} full-frame triangles")
    assert ctx.stats()["covered_pixels"] == 2 * W * H
    if (W, H) != (65, 17):
        _check_oracle(ctx, oracle_mod, _frame(W, H), a)
    if (W, H) == (64, 16):
        # the raster timeline's pair slot: the one group walked every triangle's 1,024 pairs
        ctx.set_timeline(True)
        ctx.render_batch(_frame(W, H), [a, b])
        _, _, r = ctx.debug_timeline()
        assert r[:, 9].max() == n * W * H and r[:, 8].max() == n


def _width_tris(W, H, seed):
    """One triangle per bin-box width w = 1..64, each box inside one 64x16 group of the 128x32 frame (so
    the group's clipped box is w wide), by w % 4 straddling the group's x = 32 tile seam, its y = 8 seam,
    both or neither where w allows; irregular offsets, several z layers with a tilt."""
    rng = np.random.default_rng(seed)
    tris, zs = [], []
    for w in range(1, GROUP_W + 1):
        h = int(rng.integers(2, TILE_H + 1))       # (<= 8: a box that tall can still avoid the y seam)
        over_x, over_y = bool(w & 1), bool(w & 2)
        xs = [x for x in range(0, GROUP_W - w + 1) if (x < TILE_W <= x + w - 1) == over_x]
        ys = [y for y in range(0, GROUP_H - h + 1) if (y < TILE_H <= y + h - 1) == over_y]
        if not xs:
            xs = list(range(0, GROUP_W - w + 1))
        x0 = GROUP_W * int(rng.integers(0, W // GROUP_W)) + int(rng.choice(xs))
        y0 = GROUP_H * int(rng.integers(0, H // GROUP_H)) + int(rng.choice(ys))
        x1, y1 = x0 + w - 1, y0 + h - 1          # the box: floor(min) .. floor(max)
        fx = rng.uniform(0.0, 1.0)
        tris.append([(x0 + 0.3, y0 + 0.3 + 0.4 * fx), (x1 + 0.6, y0 + 0.35), (x0 + 0.3 + fx * (x1 - x0 + 0.3), y1 + 0.6)])
        zs.append(rng.choice([0.2, 0.4, 0.6]) + rng.uniform(-0.15, 0.15, size=3))
    return _mesh_px(W, H, tris, np.asarray(zs))


def test_every_clipped_box_width(ctx, ref_ctx, oracle_mod):
    W, H = 2 * GROUP_W, 2 * GROUP_H
    fds = [[_identity_draw(_width_tris(W, H, s), s % 4)] for s in (51, 52, 53)]
    _check(ctx, ref_ctx, _frame(W, H, present=True, prequant=True), fds, "widths 1..64")
    assert ctx.stats()["covered_pixels"] > 1000
    _check_oracle(ctx, oracle_mod, _frame(W, H), fds[0])


def _wide_tris(W, H, n, seed):
    """n triangles 50-64 px wide and 5-14 px tall: each spans both tile columns of its groups."""
    rng = np.random.default_rng(seed)
    c = rng.uniform([0, 0], [W - 40, H - 6], size=(n, 1, 2))
    w, h = rng.uniform(50, 64, size=n), rng.uniform(5, 14, size=n)
    off = np.stack([np.stack([np.zeros(n), rng.uniform(0, 1, n) * h], 1), np.stack([w, rng.uniform(0, 1, n) * h], 1),
                    np.stack([rng.uniform(0.2, 0.8, n) * w, h * rng.choice([-1.0, 1.0], n)], 1)], 1)
    return _mesh_px(W, H, c + off, rng.uniform(-0.8, 0.8, size=(n, 3)))


def test_shards_leave_foreign_tiles_alone(ctx, ref_ctx, oracle_mod):
    """A shard's group has candidate pixels in tiles of other shards, which it must not touch; the batch
    under (0/1) that follows renders over the same planes."""
    W, H = 322, 181
    fds = [[_identity_draw(_wide_tris(W, H, 60, s), 3)] for s in (61, 62)]
    for i, (rank, count) in enumerate([(0, 2), (1, 2), (1, 3), (0, 1)]):
        _check(ctx, ref_ctx, _frame(W, H, shard_rank=rank, shard_count=count, present=True), fds, f"step {i}: shard {rank}/{count}")
    _check_oracle(ctx, oracle_mod, _frame(W, H), fds[0])


def _tile_clutter(W, H, tx0, ty0, n, seed):
    """n small triangles strictly inside the 32x8 tile at (tx0, ty0), z from a few values (exact ties)."""
    rng = np.random.default_rng(seed)
    c = rng.uniform([tx0 + 1, ty0 + 1], [tx0 + TILE_W - 1, ty0 + TILE_H - 1], size=(n, 1, 2))
    p = np.clip(c + rng.uniform(-5, 5, size=(n, 3, 2)), [tx0 + 0.2, ty0 + 0.2], [tx0 + TILE_W - 0.2, ty0 + TILE_H - 0.2])
    z = np.repeat(rng.choice([0.25, 0.5, -0.0, 0.0], size=(n, 1)), 3, axis=1)
    return _mesh_px(W, H, p, z)


@pytest.mark.parametrize("tile", [0, 1, 2, 3])
@pytest.mark.parametrize("W,H", [(64, 16), (322, 181)])
def test_one_busy_tile_of_four(ctx, ref_ctx, oracle_mod, W, H, tile):
    """Every pair of the group lands in one tile's key array (for tiles 1..3 not the first tile's)."""
    gx0 = GROUP_W if W > 2 * GROUP_W else 0
    gy0 = GROUP_H if H > 2 * GROUP_H else 0
    tx0, ty0 = gx0 + (tile % 2) * TILE_W, gy0 + (tile // 2) * TILE_H
    tri = _identity_draw(_mesh_px(W, H, [[(tx0 + 3.2, ty0 + 1.1), (tx0 + 25.7, ty0 + 1.8), (tx0 + 7.2, ty0 + 6.7)]], [[0.1, 0.3, -0.2]]), 3)
    draws = [tri, _identity_draw(_tile_clutter(W, H, tx0, ty0, 60, 70 + tile), 2, (0, 255, 0, 255))]
    _check(ctx, ref_ctx, _frame(W, H, present=True, prequant=True), [draws, draws[::-1]], "one busy tile")
    assert ctx.stats()["covered_pixels"] > 40
    if tile == 3:
        _check_oracle(ctx, oracle_mod, _frame(W, H), draws)


def _big_and_small_soup(W, H, n, seed):
    """n triangles over the frame (and a little beyond), a quarter of them 40-64 px across."""
    rng = np.random.default_rng(seed)
    c = rng.uniform([-10, -10], [W + 10, H + 10], size=(n, 1, 2))
    size = np.where(rng.uniform(size=n) < 0.25, rng.uniform(40, 64, size=n), rng.uniform(3, 14, size=n))
    p = c + (rng.uniform(-0.5, 0.5, size=(n, 3, 2)) * size[:, None, None])
    k = rng.integers(0, 2, size=n)                    # the enlarged ones reach their size along one axis
    i = np.arange(n)
    p[i, 0, k] = c[i, 0, k] - 0.5 * size
    p[i, 1, k] = c[i, 0, k] + 0.5 * size
    return _mesh_px(W, H, p, rng.uniform(-0.9, 0.9, size=(n, 3)))


def test_multi_round_with_large_boxes(ctx, ref_ctx, oracle_mod):
    """1,500 triangles (two gather rounds, many staging chunks: winners fetched by index) with boxes the
    group rectangle clips on all four sides."""
    W, H = 322, 181
    fds = [[_identity_draw(_big_and_small_soup(W, H, 1500, s), s % 4)] for s in (81, 82)]
    _check(ctx, ref_ctx, _frame(W, H, present=True, prequant=True), fds, "1500 triangles")
    _check_oracle(ctx, oracle_mod, _frame(W, H), fds[0])
