"""Tile groups, scalar state per phase: the group kernels hold neither their arguments nor a frame's
pointers across a work item -- every phase of raster_group (header and box scan, later scan rounds, a
staging chunk with its pair passes, the ghost fragments, the resolve loop), the item fetch and the clear
items read what they use from the kernel-argument segment and derive the frame's view from the frame
index (kernel_args / frame_view, shs_device.hpp).  A wrong stride, view or reload shows as a frame that
reads or writes another frame's records, boxes, varyings, uniforms, flags or planes.

Batches of 2-3 frames of at most 128x48 px, scan mode forced, rendered three ways -- the default context
(groups + spans), set_group_spans(False), set_tile_groups(False) -- and compared frame by frame, every
enabled plane bit for bit; one context also goes against the CPU oracle, frame by frame."""
import numpy as np
import pytest

from helpers import assert_color_parity, assert_depth_bitexact
from test_gpu_parity import _hair_soup, _identity_draw, _ndc_soup
from test_group_spans import _check3
from test_stale_clear import _frame, _planes
from test_tile_groups import GROUP_H, GROUP_W, _clutter, _mesh_px

gpu = pytest.mark.gpu

FLT_MAX = np.finfo(np.float32).max


@pytest.fixture(scope="module")
def box_ctx():
    """Tile groups whose pair pass walks whole clipped boxes."""
    import shs_gpu
    c = shs_gpu.Context(0)
    c.set_group_spans(False)
    c.set_raster_mode(1)
    yield c
    c.close()


@pytest.fixture(scope="module")
def tile_ctx():
    """Every busy tile its own work item."""
    import shs_gpu
    c = shs_gpu.Context(0)
    c.set_tile_groups(False)
    c.set_raster_mode(1)
    yield c
    c.close()


@pytest.fixture()
def ctx():
    import shs_gpu
    c = shs_gpu.Context(0)
    c.set_raster_mode(1)
    yield c
    c.close()


def _oracle_frames(c, oracle_mod, W, H, fds, frames=None, **kw):
    """The batch on context c with the prequant plane on, its frames (all, or those listed) against the
    CPU oracle's render of that frame's own draws: depth and coverage bit-exact, colour within the parity
    helper's truncation-boundary rule."""
    frame = _frame(W, H, prequant=True, **kw)
    c.render_batch(frame, fds)
    covered = 0
    for k in range(len(fds)):
        rc, rd, rpq = oracle_mod.render_legacy(W, H, fds[k], tile=frame.ref_tile, threads=8, prequant=True)
        covered += int((rd < FLT_MAX).sum())
        if frames is None or k in frames:
            gc, gd = c.resolve_frame(k)
            assert_depth_bitexact(gd, rd)
            assert_color_parity(gc, rc, c.resolve_prequant(k), rpq)
    assert c.stats()["covered_pixels"] == covered


def _soup_draw(W, H, n, seed, shading, color=(200, 120, 40, 255), kind="mixed"):
    """(The frames of a batch submit equal draw and triangle counts; their meshes are their own.)"""
    from shs_gpu.scene import Mesh
    pos, nrm = _ndc_soup(np.random.default_rng(seed), W, H, n, kind=kind)
    return _identity_draw(Mesh(pos, nrm), shading, color)


@gpu
@pytest.mark.parametrize("planes", [True, False], ids=["present+prequant", "colour+depth"])
def test_edge_groups_three_meshes(ctx, box_ctx, tile_ctx, oracle_mod, planes):
    """72x20: the last group column is one tile wide (8 px of it on the frame), the last group row one
    tile high (4 rows).  Three frames of different meshes and shadings: nothing is shared, so every frame
    reads its own recs / boxes / shade slice."""
    W, H = 72, 20
    fds = [[_soup_draw(W, H, 90, seed, sh)] for seed, sh in ((71, 3), (72, 1), (73, 2))]
    _check3(ctx, box_ctx, tile_ctx, _frame(W, H, present=planes, prequant=planes), fds, "72x20, three meshes")
    assert ctx.stats()["covered_pixels"] > W * H
    _oracle_frames(ctx, oracle_mod, W, H, fds)


@gpu
def test_static_scene_shared_varyings(ctx, box_ctx, tile_ctx, oracle_mod):
    """One mesh, shading and model matrix, a camera and a light per frame: the varyings are stored once
    (frames >= 1 read frame 0's shade records) while a winner shades with its own frame's draw uniforms."""
    from shs_gpu import scene
    W, H = 128, 48
    fds = []
    for k in range(3):
        cam = (0.9 * k - 1.0, 5.0 - 0.5 * k, -17.0 + 0.8 * k)
        _, draws = scene.monkey_scene(W, H, 3, yaw=5.0 * k - 6.0, pitch=2.0 * k - 2.5, rotation=25.0, cam_pos=cam)
        for d in draws:
            d.light_dir = np.asarray([0.4 * k - 0.5, -1.0, 0.4 + 0.2 * k], np.float32)
        fds.append(draws)
    _check3(ctx, box_ctx, tile_ctx, _frame(W, H, present=True, prequant=True), fds, "static scene")
    assert ctx.stats()["covered_pixels"] > 500
    a, b = _planes(ctx, _frame(W, H), 0), _planes(ctx, _frame(W, H), 2)
    assert not np.array_equal(a["color"], b["color"]), "the frames do not differ"
    _oracle_frames(ctx, oracle_mod, W, H, fds)


def _strip_tris(W, H, n):
    """n triangles side by side across the frame, each of them visible."""
    w = W / n
    return [[(i * w + 0.2, 1.3), ((i + 1) * w - 0.2, 2.1 + (i % 5)), (i * w + 0.5 * w, H - 1.4)] for i in range(n)]


@gpu
@pytest.mark.parametrize("n_draws", [1, 4, 33], ids=["kernel-argument table", "device table", "more draws than LDS holds"])
def test_draw_tables(ctx, box_ctx, tile_ctx, oracle_mod, n_draws):
    """2 frames x 1 draw: the draws travel as kernel arguments; x 4: the device table; x 33 one-triangle
    draws: 66 > LDS_DRAWS (64), so frame 1's last winners' uniforms come from the device table.  Every draw
    has its own colour, light and shading, and frame 1's differ from frame 0's."""
    W, H = 128, 48
    rng = np.random.default_rng(400 + n_draws)
    fds = []
    for f in range(2):
        tris = _strip_tris(W, H, max(n_draws, 8))
        per = len(tris) // n_draws
        draws = []
        for i in range(n_draws):
            mine = tris[i * per:(i + 1) * per] if i < n_draws - 1 else tris[i * per:]
            z = rng.uniform(-0.5, 0.5, size=(len(mine), 3))
            d = _identity_draw(_mesh_px(W, H, np.asarray(mine), z), (i + f) % 4, tuple(int(v) for v in rng.integers(30, 255, 3)) + (255,))
            d.light_dir = rng.uniform(-1, 1, 3).astype(np.float32)
            draws.append(d)
        fds.append(draws)
    _check3(ctx, box_ctx, tile_ctx, _frame(W, H, present=True, prequant=True), fds, f"{n_draws} draws per frame")
    _oracle_frames(ctx, oracle_mod, W, H, fds)
    col, _ = ctx.resolve_frame(1)
    assert len(np.unique(np.ascontiguousarray(col).view(np.uint32))) > n_draws, "the draws are not all visible"


@gpu
def test_second_scan_round_and_several_chunks(ctx, box_ctx, tile_ctx, oracle_mod):
    """1,100 triangles per frame need a second round of box loads (the round's own view of the boxes).  One
    frame spreads them over the screen; the other puts 130 in one group -- three staging chunks (a view per
    chunk), winners fetched by index from the frame's records in HBM -- and the rest off screen.  Frame 0
    and frame 1 swap roles between the two batches."""
    W, H = 128, 48
    big = [_soup_draw(W, H, 1000, 81, 3), _soup_draw(W, H, 100, 84, 1, (0, 90, 255, 255))]
    many = [_identity_draw(_clutter(W, H, GROUP_W, 2 * GROUP_H, 130, 82), 3, (255, 0, 0, 255)),
            _soup_draw(W, H, 970, 83, 2, (0, 255, 0, 255), kind="off")]
    frame = _frame(W, H, present=True, prequant=True)
    _check3(ctx, box_ctx, tile_ctx, frame, [big, many], "1100 | 130")
    _check3(ctx, box_ctx, tile_ctx, frame, [many, big], "130 | 1100")
    _oracle_frames(ctx, oracle_mod, W, H, [many, big])


@gpu
def test_ghost_fragments_in_frame_one_only(ctx, box_ctx, tile_ctx, oracle_mod):
    """Hair-thin slivers in frame 1 (unbounded: ghost fragments, which carry their frame) and small
    triangles in frame 0: the fragments must land in frame 1's groups and nowhere in frame 0."""
    from shs_gpu.scene import Mesh
    W, H = 128, 48
    pos, nrm = _hair_soup(np.random.default_rng(27), W, H, 2500)   # (four visible tile-clamp pixels in the oracle's render)
    fds = [[_soup_draw(W, H, 2500, 91, 3, kind="small")], [_identity_draw(Mesh(pos, nrm), 3)]]
    _check3(ctx, box_ctx, tile_ctx, _frame(W, H, present=True, prequant=True), fds, "ghosts in frame 1")
    st = ctx.stats()
    print("ghost triangles", st["tri_ghost"], "unbounded", st["tri_ghost_unbounded"], "fragments", st["ghost_fragments"])
    assert st["tri_ghost_unbounded"] > 0 and st["ghost_fragments"] > 0, "the scene has no ghost fragments"
    _oracle_frames(ctx, oracle_mod, W, H, fds)


@gpu
def test_stale_clears_of_a_later_frame(ctx, box_ctx, tile_ctx, oracle_mod):
    """A fresh context's first batch takes the full-clear path; the second batch draws elsewhere in frames 1
    and 2 (and the same in frame 0), so tiles of non-zero frames are cleared by the stale clears, through
    the clear items' own view of those frames' flags and planes."""
    W, H = 128, 48
    a = _identity_draw(_clutter(W, H, 0, 0, 40, 101), 3)                       # the group at (0, 0)
    b = _identity_draw(_clutter(W, H, GROUP_W, 2 * GROUP_H, 40, 102), 1, (20, 200, 250, 255))
    c = _identity_draw(_clutter(W, H, 0, GROUP_H, 40, 103), 2, (250, 200, 20, 255))
    frame = _frame(W, H, present=True, prequant=True)
    first, second = [[a, c], [a, c], [a, c]], [[a, c], [b, c], [a, b]]
    _check3(ctx, box_ctx, tile_ctx, frame, first, "first batch (full clear)")
    _check3(ctx, box_ctx, tile_ctx, frame, second, "second batch (stale clears)")
    clear = np.float32(FLT_MAX).view(np.uint32)
    assert (_planes(ctx, frame, 1)["depth"][:GROUP_H, :GROUP_W] == clear).all(), "frame 1's old group was not cleared"
    assert (_planes(ctx, frame, 2)["depth"][GROUP_H:2 * GROUP_H, :GROUP_W] == clear).all(), "frame 2's old group was not cleared"
    assert not (_planes(ctx, frame, 0)["depth"][:GROUP_H, :GROUP_W] == clear).all()
    _oracle_frames(ctx, oracle_mod, W, H, second)


@gpu
@pytest.mark.parametrize("rank", [0, 1])
def test_sharded_frames(ctx, box_ctx, tile_ctx, oracle_mod, rank):
    """Shard count 2: a group holds tiles of the other shard, which it must neither draw nor clear (raw
    planes compared after a batch that drew into every tile)."""
    W, H = 128, 48
    fds = [[_soup_draw(W, H, 80, 111 + k, 3 - k)] for k in range(2)]
    cover = [[_soup_draw(W, H, 30, 113, 1)], [_soup_draw(W, H, 30, 114, 1)]]
    _check3(ctx, box_ctx, tile_ctx, _frame(W, H, present=True), cover, "unsharded")
    _check3(ctx, box_ctx, tile_ctx, _frame(W, H, shard_rank=rank, shard_count=2, present=True), fds, f"shard {rank}/2", raw=True)
    _check3(ctx, box_ctx, tile_ctx, _frame(W, H, present=True), fds, "unsharded after the shard")
    _oracle_frames(ctx, oracle_mod, W, H, fds)


@gpu
def test_timeline_build_same_images_and_slots(ctx, box_ctx, oracle_mod):
    """The timeline's marks are an instantiation of their own: its images are the plain kernel's, and slots
    9 (pairs; spans walk fewer than whole boxes), 12 (busy tiles of the first group) and 13 (span pass
    marked; 0 for whole boxes) of a one-group batch are what the whole-box context reports."""
    W, H = GROUP_W, GROUP_H
    draws = [_identity_draw(_clutter(W, H, 0, 0, 40, 121), 3), _identity_draw(_clutter(W, H, 0, 0, 10, 122), 0, (9, 250, 90, 255))]
    frame = _frame(W, H, present=True, prequant=True)
    ctx.render_batch(frame, [draws, draws[::-1]])
    plain = [_planes(ctx, frame, k) for k in range(2)]
    rows = {}
    for name, c in (("spans", ctx), ("boxes", box_ctx)):
        c.set_timeline(True)
        try:
            c.render_batch(frame, [draws, draws[::-1]])
            _, _, rows[name] = c.debug_timeline()
        finally:
            c.set_timeline(False)
        for k in range(2):
            got = _planes(c, frame, k)
            for plane in plain[k]:
                assert np.array_equal(got[plane], plain[k][plane]), f"timeline on ({name}): frame {k}: {plane} differs"
    r, r0 = rows["spans"], rows["boxes"]
    print("pairs", int(r[:, 9].max()), "whole boxes", int(r0[:, 9].max()), "busy tiles", int(r[:, 12].max()))
    covered = ctx.stats()["covered_pixels"] // 2
    assert covered <= int(r[:, 9].max()) <= int(r0[:, 9].max())
    assert int(r[:, 12].max()) == int(r0[:, 12].max()) == 4
    assert r[:, 13].max() > 0 and (r0[:, 13] == 0).all()
    assert int(r[:, 8].max()) == int(r0[:, 8].max()) == 50, "candidates of the group"
    ctx.render_batch(frame, [draws, draws[::-1]])     # and back to the plain kernel
    for k in range(2):
        got = _planes(ctx, frame, k)
        for plane in plain[k]:
            assert np.array_equal(got[plane], plain[k][plane]), f"timeline off again: frame {k}: {plane} differs"
    _oracle_frames(ctx, oracle_mod, W, H, [draws, draws[::-1]])
