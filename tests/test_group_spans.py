"""Tile groups, row-span pair tasks (SHS_OPT_LEGACY_GROUP_SPANS): a busy 2x2 group (64x16 px) cuts every
staged candidate's box, clipped to the group rectangle, into its rows, keeps of each row only the
conservative span legacy_row_span gives (every pixel that can pass the reference's barycentric test lies
inside it) and lays the nonempty spans end to end as segments; a pair finds its pixel from its segment.
The pairs tested are a superset of the passing ones, so the images are the whole-box pass's bits.  A
staging chunk whose spans hold more pairs than the 16,384-pair bitmap takes the box passes.

GPU tests: the default context (spans), one with set_group_spans(False) (whole boxes) and one with
set_tile_groups(False) (a work item per tile) render the same batches of >= 2 frames, scan mode forced;
every frame and every enabled plane is compared bit for bit.  One case per test also goes against the
CPU oracle.  CPU tests: the numpy restatement of legacy_row_span over group-sized clips, and the segment
word's layout."""
import numpy as np
import pytest

from test_gpu_parity import _identity_draw, _ndc_soup
from test_group_pairs import _full_frame_tris, _wide_tris, _width_tris
from test_legacy_row_spans import _inside_vec, _record, legacy_span
from test_stale_clear import _frame, _hair_sets, _planes
from test_tile_groups import GROUP_H, GROUP_W, _check_oracle, _clutter, _cover_draw, _mesh_px

gpu = pytest.mark.gpu

SEAM_SIZES = [(64, 16), (128, 32)]       # whole groups: boxes straddle the x = 32 and y = 8 tile seams
EDGE_SIZES = [(65, 17), (96, 24)]        # edge groups of one tile column or row, partial tiles
PAIR_CAP = 16384                         # pairs one pass lays out (shs_legacy.hip)


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


def _check3(c, box, tile, frame, fds, label="", raw=False):
    """Render the batch on the three contexts; every frame, every enabled plane, bit-exact.  raw: the
    planes as they are, other shards' pixels included."""
    for x in (c, box, tile):
        x.render_batch(frame, fds)
    view = _frame(frame.width, frame.height, present=frame.present, prequant=frame.prequant) if raw else frame
    for k in range(len(fds)):
        got = _planes(c, view, k)
        for name, other in (("whole boxes", box), ("a work item per tile", tile)):
            want = _planes(other, view, k)
            for plane in want:
                assert np.array_equal(got[plane], want[plane]), f"{label}: frame {k}: {plane} differs from {name}"


# ---- GPU ------------------------------------------------------------------------------------------


@gpu
@pytest.mark.parametrize("W,H", SEAM_SIZES + EDGE_SIZES)
def test_every_clipped_width(ctx, box_ctx, tile_ctx, oracle_mod, W, H):
    """(a, b) One triangle per clipped box width 1..64, straddling the tile seams by turns."""
    fds = [[_identity_draw(_width_tris(W, H, s), s % 4)] for s in (51, 52, 53)]
    _check3(ctx, box_ctx, tile_ctx, _frame(W, H, present=True, prequant=True), fds, "widths 1..64")
    assert ctx.stats()["covered_pixels"] > 300
    if (W, H) in ((128, 32), (96, 24)):
        _check_oracle(ctx, oracle_mod, _frame(W, H), fds[0])


def _exact_tris(W, H, n, seed):
    """Triangles whose pixels sit on the barycentric test's boundary: corners on pixel centres (edges
    through centres), integer corners (45-degree edges through centres), slivers a corner ~1e-3 px off
    the opposite edge, and hair-thin ones across the whole frame; both windings."""
    from shs_gpu.scene import Mesh
    rng = np.random.default_rng(seed)
    tris = []
    for i in range(n):
        kind = i % 4
        base = rng.uniform([0, 0], [W, H])
        if kind == 0:
            p = np.round(base + rng.uniform(-9, 9, (3, 2))) + 0.5
        elif kind == 1:
            k = int(rng.integers(2, 9))
            b = np.round(base)
            p = np.array([b, b + [k, k], b + [k, -k]]) if i % 8 == 1 else np.array([b, b + [2 * k, 0], b + [0, k]])
        elif kind == 2:
            d = rng.uniform(-30, 30, 2)
            p = np.array([base, base + d, base + d * rng.uniform(0.2, 0.8) + rng.normal(0, 1e-3, 2)])
        else:
            d = rng.uniform([-W, -H], [W, H])
            p = np.array([base, base + d, base + d * rng.uniform(0.1, 0.9) + rng.normal(0, 1e-2, 2)])
        tris.append(p)
    m = _mesh_px(W, H, np.asarray(tris), rng.uniform(-0.8, 0.8, size=(n, 3)))
    pos = m.positions.reshape(-1, 3, 3).copy()
    nrm = m.normals.reshape(-1, 3, 3).copy()
    pos[1::2] = pos[1::2][:, [0, 2, 1]]      # the other winding
    nrm[1::2] = nrm[1::2][:, [0, 2, 1]]
    return Mesh(pos.reshape(-1, 9), nrm.reshape(-1, 9))


@gpu
@pytest.mark.parametrize("W,H", SEAM_SIZES + EDGE_SIZES)
def test_pixels_on_the_edges_survive(ctx, box_ctx, tile_ctx, oracle_mod, W, H):
    """(c) A barycentric of exactly 0 passes: the span must keep such pixels."""
    fds = [[_identity_draw(_exact_tris(W, H, 120, s), 3)] for s in (5, 6)]
    _check3(ctx, box_ctx, tile_ctx, _frame(W, H, present=True, prequant=True), fds, "edge pixels")
    assert ctx.stats()["covered_pixels"] > 100
    if (W, H) in ((64, 16), (65, 17)):
        _check_oracle(ctx, oracle_mod, _frame(W, H), fds[0])


@gpu
def test_sliver_soup_ghosts_and_tile_clamp(ctx, box_ctx, tile_ctx, oracle_mod):
    """(d) 168x88: three 80x80 reference-tile columns and two rows.  The tile clamp makes slivers visit
    pixels outside their bbox -- the oracle's 80x80-tile render of frame 1 differs from its single-tile
    render -- and ghost candidates' expanded bin boxes are walked by spans."""
    W, H = 168, 88
    A, B = _hair_sets(W, H, 2, 3000, 500)
    frame = _frame(W, H, present=True, prequant=True)
    _check3(ctx, box_ctx, tile_ctx, frame, A, "A")
    st = ctx.stats()
    print("ghost triangles", st["tri_ghost"], "unbounded", st["tri_ghost_unbounded"], "fragments", st["ghost_fragments"])
    assert st["tri_ghost"] > 0 and st["tri_ghost_unbounded"] > 0
    _check3(ctx, box_ctx, tile_ctx, frame, B, "B")
    _, d80, _ = oracle_mod.render_legacy(W, H, A[1], tile=(80, 80), threads=8)
    _, d1, _ = oracle_mod.render_legacy(W, H, A[1], tile=(W, H), threads=8)
    assert not np.array_equal(d80.view(np.uint32), d1.view(np.uint32)), "scene has no tile-clamp ghost pixels"
    _check_oracle(ctx, oracle_mod, _frame(W, H), A[1])


@gpu
@pytest.mark.parametrize("W,H", SEAM_SIZES + EDGE_SIZES)
def test_chunks_and_gather_rounds(ctx, box_ctx, tile_ctx, oracle_mod, W, H):
    """(e) 70 and 130 small candidates in one group (two and three staging chunks), then a frame of 1,100
    triangles (two gather rounds): the winners are fetched by index."""
    from shs_gpu.scene import Mesh
    frame = _frame(W, H, present=True, prequant=True)
    for n in (70, 130):
        draws = [_identity_draw(_clutter(W, H, 0, 0, n - 30, 20 + n), 3, (255, 0, 0, 255)),
                 _identity_draw(_clutter(W, H, 0, 0, 30, 21 + n), 2, (0, 255, 0, 255))]
        _check3(ctx, box_ctx, tile_ctx, frame, [draws, draws[::-1]], f"{n} candidates")
    fds = []
    for seed in (33, 34):
        pos, nrm = _ndc_soup(np.random.default_rng(seed), W, H, 1100)
        fds.append([_identity_draw(Mesh(pos, nrm), seed % 4)])
    _check3(ctx, box_ctx, tile_ctx, frame, fds, "1100 triangles")
    if (W, H) in ((128, 32), (96, 24)):
        _check_oracle(ctx, oracle_mod, _frame(W, H), fds[0])


@gpu
@pytest.mark.parametrize("case", ["24", "70", "mixed"])
def test_more_span_pairs_than_the_bitmap_holds(ctx, box_ctx, tile_ctx, oracle_mod, case):
    """(f) Full-frame triangles' spans are whole rows: 24 of them make 24,576 span pairs, so the chunk
    takes the box passes; 70: the first chunk does, the second (6,144 pairs) walks spans; a chunk of 20
    full-frame and 40 small triangles falls back as a whole."""
    W, H = 64, 16
    if case == "mixed":
        a = [_identity_draw(_full_frame_tris(W, H, 20, 91), 3), _identity_draw(_clutter(W, H, 0, 0, 40, 92), 1, (30, 220, 90, 255))]
        b = a[::-1]
    else:
        n = int(case)
        a = [_identity_draw(_full_frame_tris(W, H, n, 40 + n), 3)]
        b = [_identity_draw(_full_frame_tris(W, H, n, 41 + n), 1, (30, 220, 90, 255))]
    _check3(ctx, box_ctx, tile_ctx, _frame(W, H, present=True, prequant=True), [a, b], f"{case} full-frame triangles")
    assert ctx.stats()["covered_pixels"] == 2 * W * H
    if case != "70":
        _check_oracle(ctx, oracle_mod, _frame(W, H), a)


@gpu
@pytest.mark.parametrize("W,H", SEAM_SIZES + EDGE_SIZES)
def test_shards_leave_foreign_tiles_alone(ctx, box_ctx, tile_ctx, oracle_mod, W, H):
    """(g) Two shards: a group's tile columns belong to different shards.  After a batch that drew into
    every tile, each shard's batch must leave the other shard's pixels as they were (raw planes compared)."""
    fds = [[_identity_draw(_wide_tris(W, H, 30, s), 3)] for s in (61, 62)]
    cover = [[_cover_draw(W, H)], [_cover_draw(W, H)]]
    for rank in (0, 1):
        _check3(ctx, box_ctx, tile_ctx, _frame(W, H, present=True), cover, "every tile busy")
        _check3(ctx, box_ctx, tile_ctx, _frame(W, H, shard_rank=rank, shard_count=2, present=True), fds, f"shard {rank}/2", raw=True)
    _check3(ctx, box_ctx, tile_ctx, _frame(W, H, present=True), fds, "unsharded after the shards")
    if (W, H) == (128, 32):
        _check_oracle(ctx, oracle_mod, _frame(W, H), fds[0])


@gpu
def test_timeline_counts_span_pairs(ctx, box_ctx, oracle_mod):
    """(h) The raster timeline's pair slot counts the pairs walked.  A right triangle (2.25, 1.25),
    (50.25, 1.25), (2.25, 13.25): row py = 1..12 passes px = 2 .. 52 - 4 py (every centre >= 0.25 px from
    an edge), 300 pixels in a 49x13 box.  Full-frame triangles' spans are their rows."""
    W, H = 64, 16
    tri = [_identity_draw(_mesh_px(W, H, [[(2.25, 1.25), (50.25, 1.25), (2.25, 13.25)]], [[0.1, 0.3, -0.2]]), 3)]
    passing, box = sum(51 - 4 * py for py in range(1, 13)), 49 * 13
    assert passing == 300
    for c in (ctx, box_ctx):
        c.set_timeline(True)
    try:
        ctx.render_batch(_frame(W, H), [tri, tri])
        assert ctx.stats()["covered_pixels"] == 2 * passing
        _, _, r = ctx.debug_timeline()
        pairs = int(r[:, 9].max())
        print("right triangle: span pairs", pairs, "passing", passing, "box", box)
        assert passing <= pairs <= box
        assert pairs <= passing + 4 * 12, "a row's span is at most two pixels wider on either side"
        assert r[:, 13].max() > 0, "no span pass was marked"
        box_ctx.render_batch(_frame(W, H), [tri, tri])
        _, _, r0 = box_ctx.debug_timeline()
        assert int(r0[:, 9].max()) == box and (r0[:, 13] == 0).all()
        for n in (10, 24):     # 10,240 span pairs: spans; 24,576: the box passes
            full = [_identity_draw(_full_frame_tris(W, H, n, 40 + n), 3)]
            ctx.render_batch(_frame(W, H), [full, full])
            _, _, r = ctx.debug_timeline()
            assert int(r[:, 9].max()) == n * W * H and int(r[:, 8].max()) == n
    finally:
        box_ctx.set_timeline(False)
    _check_oracle(ctx, oracle_mod, _frame(W, H), tri)


# ---- CPU ------------------------------------------------------------------------------------------


def _seam_triangles(rng, n):
    """(corners, regular) -- random, sliver, hair-thin and centre-aligned triangles placed on group seams
    (x = 64 k, y = 16 k); regular: a plain random triangle (not a sliver, not hair-thin)."""
    for it in range(n):
        kind = it % 5
        seam = np.array([64.0 * rng.integers(1, 20), 16.0 * rng.integers(1, 40)])
        base = seam + rng.uniform(-12, 12, 2)
        if kind == 0:
            pts = base + rng.uniform(-10, 10, (3, 2))
        elif kind == 1:
            pts = base + rng.uniform(-45, 45, (3, 2))
        elif kind == 2:   # sliver: a corner within ~1e-3 px of the opposite edge
            d = rng.uniform(-30, 30, 2)
            pts = np.array([base, base + d, base + d * rng.uniform(0.2, 0.8) + rng.normal(0, 1e-3, 2)])
        elif kind == 3:   # hair-thin and long
            d = rng.uniform(-300, 300, 2)
            pts = np.array([base, base + d, base + d * rng.uniform(0.1, 0.9) + rng.normal(0, 1e-4, 2)])
        else:
            pts = base + rng.uniform(-25, 25, (3, 2))
        if it % 3 == 0:
            pts = np.round(pts) + 0.5   # corners on pixel centres: edges through centres
        elif it % 3 == 1:
            pts = np.round(pts)
        if rng.uniform() < 0.5:
            pts = pts[::-1]             # both windings
        yield pts.astype(np.float32), kind in (0, 1, 4)


def test_group_row_spans_hold_every_passing_pixel():
    """legacy_row_span over group clips (<= 64 wide, <= 16 rows): no passing pixel outside its row's span,
    for the bbox clipped to each group it overlaps and, as for a ghost's expanded box, the whole group.
    The spans must also cut: over the plain random triangles' bbox clips the pixels tested stay <= 1.6x
    the passing ones (a row costs <= ~2 pixels of margin on either side; whole rows would be ~2.5x+)."""
    rng = np.random.default_rng(0x5EA5)
    missed = passing_all = tested_reg = passing_reg = n_tris = 0
    for pts, regular in _seam_triangles(rng, 3500):
        rec = _record(pts)
        if not abs(rec[-1]) >= 1e-5:    # barycentric_coordinate rejects every pixel
            continue
        n_tris += 1
        bx0, bx1 = int(np.floor(pts[:, 0].min())), int(np.floor(pts[:, 0].max()))
        by0, by1 = int(np.floor(pts[:, 1].min())), int(np.floor(pts[:, 1].max()))
        groups = [(gx, gy) for gy in range(by0 // GROUP_H, by1 // GROUP_H + 1) for gx in range(bx0 // GROUP_W, bx1 // GROUP_W + 1)][:4]
        for gi, (gx, gy) in enumerate(groups):
            GX0, GY0 = gx * GROUP_W, gy * GROUP_H
            whole = gi == 0 and n_tris % 4 == 0          # a ghost's expanded box: the group rectangle
            x0, x1 = (GX0, GX0 + GROUP_W - 1) if whole else (max(bx0, GX0), min(bx1, GX0 + GROUP_W - 1))
            y0, y1 = (GY0, GY0 + GROUP_H - 1) if whole else (max(by0, GY0), min(by1, GY0 + GROUP_H - 1))
            xs = np.arange(x0, x1 + 1)
            for py in range(y0, y1 + 1):
                s0, s1 = legacy_span(rec, py, x0, x1)
                ok = _inside_vec(rec, xs, np.full(len(xs), py))
                missed += int((ok & ((xs < s0) | (xs > s1))).sum())
                passing_all += int(ok.sum())
                if regular and not whole:
                    tested_reg += max(0, s1 - s0 + 1)
                    passing_reg += int(ok.sum())
    assert n_tris >= 3000
    assert missed == 0, f"{missed} of {passing_all} passing pixels outside their row span"
    print(f"plain triangles: {tested_reg} tested / {passing_reg} passing = {tested_reg / passing_reg:.3f}")
    assert passing_reg > 50000
    assert tested_reg <= 1.6 * passing_reg, "the spans cut too little"


def _seg_pack(first, x0, row, cand):
    """seg_pack (shs_legacy.hip): first pair | x0 << 14 | row << 20 | candidate << 24."""
    return first | (x0 << 14) | (row << 20) | (cand << 24)


def test_segment_word_round_trip():
    x0, row, cand = np.meshgrid(np.arange(64, dtype=np.uint64), np.arange(16, dtype=np.uint64), np.arange(64, dtype=np.uint64),
                                indexing="ij")
    for first in (0, 1, 63, 64, 4095, 8192, PAIR_CAP - 64, PAIR_CAP - 1):
        w = _seg_pack(np.uint64(first), x0, row, cand)
        assert (w < 2 ** 32).all()
        w = w.astype(np.uint32)
        assert ((w & 0x3fff) == first).all()
        assert (((w >> 14) & 63) == x0).all() and (((w >> 20) & 15) == row).all() and ((w >> 24) == cand).all()
    assert len(np.unique(_seg_pack(np.uint64(PAIR_CAP - 1), x0, row, cand))) == 64 * 16 * 64
