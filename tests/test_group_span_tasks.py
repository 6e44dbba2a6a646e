"""Tile groups, the span pass's tasks (shs_legacy.hip raster_group, SHS_OPT_LEGACY_GROUP_SPANS): one task
per (staged candidate, group row of its bin box clipped to the group), dealt over the workgroup in rounds of
256.  The staged candidates with rows (the entries, by rank) lie end to end after one wave prefix -- at most
64 x 16 = 1,024 tasks -- with each entry's start in a bitmap over the tasks and the entry owning every
bitmap word's first task; task t finds its entry from its word (first owner + the starts up to it) and its
row from the entry's first task.  The row-independent part of legacy_row_span (span_terms) is computed once
per entry, the row part (span_row) per task: the same operations on the same operands, so the spans -- and
with them the pairs and the images -- are the same bits as the one-piece evaluation's.

GPU tests: test_group_spans.py's three contexts (spans, whole boxes, a work item per tile) render the same
batches of >= 2 frames, scan mode forced; every frame and every enabled plane is compared bit for bit, and
one case per test also goes against the CPU oracle.  The shapes are those where the dealing can go wrong:
task counts at the word and round boundaries, row ranges cut by the group, edge groups, several staging
chunks, the overflow to the box passes, ghosts' expanded boxes and a sharded frame.  CPU tests: numpy
restatements of the dealing and of the split evaluation."""
import numpy as np
import pytest

from test_group_pairs import _full_frame_tris, _wide_tris
from test_group_spans import _check3, _check_oracle, _frame, _hair_sets, _identity_draw, _mesh_px
from test_gpu_parity import _ndc_soup
from test_legacy_row_spans import _record, _triangles, legacy_span
from test_tile_groups import GROUP_H, GROUP_W, _clutter, _cover_draw

gpu = pytest.mark.gpu
f = np.float32

MAX_CANDS = 64                       # staged candidates per chunk (RCHUNK)
MAX_TASKS = MAX_CANDS * GROUP_H      # 1,024
PAIR_CAP = 16384


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


# ---- scenes ---------------------------------------------------------------------------------------
# Corners sit 0.2 .. 0.8 px inside their pixels, so the bin boxes (floor of the float bbox; an ordinary
# triangle's ghost expansion is ~1e-5 px) are the stated ones.


def _tall(x0, w, y0=0, y1=GROUP_H - 1):
    """A triangle whose box is columns x0 .. x0 + w - 1, rows y0 .. y1."""
    return [(x0 + 0.2, y0 + 0.3), (x0 + w - 0.2, y0 + 0.4), (x0 + 0.5 * w, y1 + 0.7)]


def _one_row(x0, w, row):
    """A triangle whose float bbox is columns x0 .. x0 + w - 1 of one row (it holds the row's pixel centres).
    Up to w = 6 that is its bin box too; a wider one is a sliver whose bin box is expanded (a ghost)."""
    return [(x0 + 0.2, row + 0.25), (x0 + w - 0.2, row + 0.3), (x0 + 0.5 * w, row + 0.8)]


def _draws(W, H, tris, seed, shading=3):
    rng = np.random.default_rng(seed)
    z = rng.choice([0.2, 0.4, 0.6], size=(len(tris), 1)) + rng.uniform(-0.15, 0.15, size=(len(tris), 3))
    return [_identity_draw(_mesh_px(W, H, np.asarray(tris, np.float64), z), shading)]


def _boundary_tris(n, extra):
    """n full-height triangles (16 tasks each) side by side in the 64x16 frame, plus `extra` one-row ones."""
    w = min(3, GROUP_W // n)
    tris = [_tall(i * (GROUP_W // n), w) for i in range(n)]
    return tris + [_one_row(40, 6, 5 + 4 * k) for k in range(extra)], n * w * GROUP_H + extra * 6


def _pairs_of_single_group(c, frame, draws):
    """The timeline's (pairs walked, span passes marked) of a batch of two equal one-group frames."""
    c.set_timeline(True)
    try:
        c.render_batch(frame, [draws, draws])
        covered = c.stats()["covered_pixels"] // 2
        _, _, r = c.debug_timeline()
    finally:
        c.set_timeline(False)
    return int(r[:, 9].max()), int(r[:, 13].max()), covered


# ---- GPU ------------------------------------------------------------------------------------------


@gpu
@pytest.mark.parametrize("n,extra", [(4, 0), (4, 1), (16, 0), (16, 1), (64, 0)], ids=["64", "65", "256", "257", "1024"])
def test_task_count_boundaries(ctx, box_ctx, tile_ctx, oracle_mod, n, extra):
    """64 tasks fill one bitmap word, 65 start the next; 256 fill one round, 257 start the second; 1,024
    are four full rounds, the most a chunk can hold."""
    W, H = GROUP_W, GROUP_H
    tris, box_px = _boundary_tris(n, extra)
    a, b = _draws(W, H, tris, 10 + n), _draws(W, H, tris[::-1], 11 + n, shading=1)
    _check3(ctx, box_ctx, tile_ctx, _frame(W, H, present=True, prequant=True), [a, b], f"{16 * n + extra} tasks")
    pairs, spans, covered = _pairs_of_single_group(ctx, _frame(W, H), a)
    print("tasks", 16 * n + extra, "pairs", pairs, "covered", covered, "box pixels", box_px)
    assert covered > 0 and spans > 0, "no span pass was marked"
    assert covered <= pairs <= box_px          # (every covered pixel passed: passing >= covered)
    assert _pairs_of_single_group(box_ctx, _frame(W, H), a) == (box_px, 0, covered)   # whole boxes: no span pass
    if extra or n == 64:
        _check_oracle(ctx, oracle_mod, _frame(W, H), a)


@gpu
def test_row_ranges(ctx, box_ctx, tile_ctx, oracle_mod):
    """One-row candidates on the group's first and last rows and on either side of its tile seam; in a
    64x48 frame boxes that start above a group and end inside it, the reverse, and boxes through a whole
    group -- across both group seams."""
    W, H = GROUP_W, GROUP_H
    rows = [_one_row(3 + 15 * k + 4 * j, 3, r) for k, r in enumerate((0, 7, 8, 15)) for j in range(3)]
    a, b = _draws(W, H, rows, 1), _draws(W, H, rows[::-1], 2, shading=2)
    _check3(ctx, box_ctx, tile_ctx, _frame(W, H, present=True, prequant=True), [a, b], "one-row candidates")
    pairs, spans, covered = _pairs_of_single_group(ctx, _frame(W, H), a)
    assert covered > 0 and spans > 0 and covered <= pairs <= len(rows) * 3
    assert _pairs_of_single_group(box_ctx, _frame(W, H), a) == (len(rows) * 3, 0, covered)   # one-row boxes, 3 px
    _check_oracle(ctx, oracle_mod, _frame(W, H), a)
    W, H = GROUP_W, 3 * GROUP_H
    tris = [_tall(1, 5, 10, 20), _tall(8, 4, 15, 16), _tall(14, 6, 28, 40), _tall(22, 3, 31, 32), _tall(27, 7, 5, 45),
            _tall(36, 2, 16, 31), _tall(40, 5, 0, 15), _tall(47, 6, 12, 35), _tall(55, 8, 33, 47), _one_row(2, 60, 16),
            _one_row(1, 62, 31)]
    a, b = _draws(W, H, tris, 3), _draws(W, H, [[(x, H - y) for x, y in t] for t in tris], 4, shading=1)
    _check3(ctx, box_ctx, tile_ctx, _frame(W, H, present=True, prequant=True), [a, b], "group seams")
    assert ctx.stats()["covered_pixels"] > 100
    _check_oracle(ctx, oracle_mod, _frame(W, H), a)


@gpu
@pytest.mark.parametrize("W,H", [(65, 17), (96, 24)])
def test_edge_groups(ctx, box_ctx, tile_ctx, oracle_mod, W, H):
    """Groups of one tile column or row, and partial tiles: boxes that reach the frame's last row and
    column (and triangles that go past them) get no task for a row the frame does not have."""
    tris = [_tall(x0, 4, y0, H + 6) for x0, y0 in ((2, 3), (30, 10), (60, 0), (W - 3, 14))]
    tris += [_tall(x0, 5, 9, H - 1) for x0 in (10, 40, W - 6)]
    tris += [_one_row(W - 12, 18, H - 1), _one_row(50, 20, 16), [(W - 9.5, 2.5), (W + 30.0, 8.0), (W - 7.5, H + 9.0)]]
    a = _draws(W, H, tris, 7) + [_identity_draw(_clutter(W, H, W - GROUP_W, H - GROUP_H, 40, 8), 1, (30, 220, 90, 255))]
    b = [_identity_draw(_clutter(W, H, 0, 0, 40, 9), 3)] + _draws(W, H, tris[::-1], 10, shading=2)
    _check3(ctx, box_ctx, tile_ctx, _frame(W, H, present=True, prequant=True), [a, b], "edge groups")
    assert ctx.stats()["covered_pixels"] > 100
    _check_oracle(ctx, oracle_mod, _frame(W, H), a)


@gpu
def test_chunks_and_gather_rounds(ctx, box_ctx, tile_ctx, oracle_mod):
    """65, 70 and 128 candidates in one group: two staging chunks, each with its own task prefix, the keys
    kept across them (65: a second chunk of one candidate).  Then 1,100 small triangles in 128x32: two
    gather rounds."""
    from shs_gpu.scene import Mesh
    W, H = GROUP_W, GROUP_H
    frame = _frame(W, H, present=True, prequant=True)
    for n in (65, 70, 128):
        draws = [_identity_draw(_clutter(W, H, 0, 0, n - 30, 20 + n), 3, (255, 0, 0, 255)),
                 _identity_draw(_clutter(W, H, 0, 0, 30, 21 + n), 2, (0, 255, 0, 255))]
        _check3(ctx, box_ctx, tile_ctx, frame, [draws, draws[::-1]], f"{n} candidates")
        if n == 65:
            _check_oracle(ctx, oracle_mod, _frame(W, H), draws)
    W, H = 2 * GROUP_W, 2 * GROUP_H
    fds = []
    for seed in (35, 36):
        pos, nrm = _ndc_soup(np.random.default_rng(seed), W, H, 1100, kind="small")
        fds.append([_identity_draw(Mesh(pos, nrm), seed % 4)])
    _check3(ctx, box_ctx, tile_ctx, _frame(W, H, present=True, prequant=True), fds, "1100 triangles")
    assert ctx.stats()["covered_pixels"] > 1000


@gpu
@pytest.mark.parametrize("n", [24, 70])
def test_overflow_takes_the_box_passes(ctx, box_ctx, tile_ctx, oracle_mod, n):
    """24 full-frame triangles: 384 tasks whose spans are whole rows, 24,576 pairs -- the chunk falls back
    to the box passes.  70: the first chunk (64) falls back, the second (6 triangles, 6,144 pairs) walks
    spans again."""
    W, H = GROUP_W, GROUP_H
    a = [_identity_draw(_full_frame_tris(W, H, n, 40 + n), 3)]
    b = [_identity_draw(_full_frame_tris(W, H, n, 41 + n), 1, (30, 220, 90, 255))]
    _check3(ctx, box_ctx, tile_ctx, _frame(W, H, present=True, prequant=True), [a, b], f"{n} full-frame triangles")
    assert ctx.stats()["covered_pixels"] == 2 * W * H
    pairs, spans, covered = _pairs_of_single_group(ctx, _frame(W, H), a)
    assert covered == W * H and pairs == n * W * H      # boxes and whole-row spans alike: every pixel of every triangle
    if n == 24:
        _check_oracle(ctx, oracle_mod, _frame(W, H), a)


@gpu
def test_ghosts_expanded_boxes(ctx, box_ctx, tile_ctx, oracle_mod):
    """The 168x88 sliver soup: ghost candidates' bin boxes are expanded past their float bboxes (read from
    the staged ext records), and their tasks cover the expanded rows."""
    W, H = 168, 88
    A, B = _hair_sets(W, H, 2, 3000, 500)
    frame = _frame(W, H, present=True, prequant=True)
    _check3(ctx, box_ctx, tile_ctx, frame, A, "A")
    st = ctx.stats()
    assert st["tri_ghost"] > 0 and st["tri_ghost_unbounded"] > 0
    _check3(ctx, box_ctx, tile_ctx, frame, B, "B")
    _check_oracle(ctx, oracle_mod, _frame(W, H), B[0])


@gpu
def test_two_shard_frame(ctx, box_ctx, tile_ctx, oracle_mod):
    """Two shards: some of a group's tiles belong to the other shard, whose pixels must stay as they were
    (raw planes compared) while every candidate's rows are still dealt."""
    W, H = 2 * GROUP_W, 2 * GROUP_H
    fds = [[_identity_draw(_wide_tris(W, H, 30, s), 3)] for s in (71, 72)]
    cover = [[_cover_draw(W, H)], [_cover_draw(W, H)]]
    for rank in (0, 1):
        _check3(ctx, box_ctx, tile_ctx, _frame(W, H, present=True), cover, "every tile busy")
        _check3(ctx, box_ctx, tile_ctx, _frame(W, H, shard_rank=rank, shard_count=2, present=True), fds, f"shard {rank}/2", raw=True)
    _check3(ctx, box_ctx, tile_ctx, _frame(W, H, present=True), fds, "unsharded after the shards")
    _check_oracle(ctx, oracle_mod, _frame(W, H), fds[1])


# ---- CPU ------------------------------------------------------------------------------------------


def _span_entry(first, row0, x0, x1, cand):
    """span_entry (shs_legacy.hip): first task | first row << 10 | x0 << 14 | x1 << 20 | candidate << 26."""
    return first | (row0 << 10) | (x0 << 14) | (x1 << 20) | (cand << 26)


def _deal(y0, y1):
    """The span pass's dealing for staged candidates with clipped group rows y0[c] .. y1[c] (none when y0 >
    y1): row counts -> inclusive prefix -> entries by rank, start bitmap and word owners -> per task its
    (candidate, row).  Returns the tasks in task order."""
    m = len(y0)
    assert 1 <= m <= MAX_CANDS
    rows = np.maximum(0, np.asarray(y1) - np.asarray(y0) + 1)
    incl = np.cumsum(rows)
    total = int(incl[-1])
    on = rows > 0
    rank = np.cumsum(on) - on                      # lanes_below(ballot(rows > 0))
    bits = [0] * (MAX_TASKS // 64)
    town = [None] * (MAX_TASKS // 64)              # (words no run reaches are never read)
    entry = {}
    for c in range(m):
        if not on[c]:
            continue
        start, e = int(incl[c] - rows[c]), int(rank[c])
        entry[e] = _span_entry(start, int(y0[c]), 0, 0, c)
        bits[start >> 6] |= 1 << (start & 63)      # mark_run
        wd = (start + 63) >> 6
        while wd * 64 < start + int(rows[c]):
            town[wd] = e
            wd += 1
    out = []
    for rnd in range((total + 255) // 256):        # block-uniform rounds of 256 threads
        for tid in range(256):
            t = 256 * rnd + tid
            if t >= total:
                continue
            word, lane = t >> 6, t & 63            # (a wave's 64 tasks: one word)
            upto = ((2 << lane) - 1) & ~1
            e = town[word] + bin(bits[word] & upto).count("1")    # pair_owner
            en = entry[e]
            out.append((en >> 26, t - (en & 1023) + ((en >> 10) & 15)))
    return out, total


def _check_deal(y0, y1):
    got, total = _deal(y0, y1)
    want = [(c, r) for c in range(len(y0)) for r in range(y0[c], y1[c] + 1)]
    assert total == len(want) <= MAX_TASKS
    assert got == want, "every (candidate, row) exactly once, candidate-major"


def _ranges_with_total(rng, total):
    """Random clipped row ranges (some empty) whose row counts sum to `total`."""
    m = int(rng.integers(max(1, -(-total // GROUP_H)), MAX_CANDS + 1))
    rows = np.zeros(m, np.int64)
    while rows.sum() < total:
        c = int(rng.integers(0, m))
        rows[c] += rows[c] < GROUP_H
    y0 = np.array([int(rng.integers(0, GROUP_H - r + 1)) for r in rows])
    y0[rows == 0] = rng.integers(1, GROUP_H, size=int((rows == 0).sum()))
    return y0, y0 + rows - 1


def test_dealing_every_task_exactly_once():
    rng = np.random.default_rng(0xDEA1)
    for total in (0, 1, 63, 64, 65, 256, 257, 1024):
        for _ in range(6):
            _check_deal(*_ranges_with_total(rng, total))
    for _ in range(300):
        m = int(rng.integers(1, MAX_CANDS + 1))
        y0 = rng.integers(0, GROUP_H, size=m)
        y1 = np.where(rng.uniform(size=m) < 0.2, y0 - 1, rng.integers(y0, GROUP_H))   # a fifth without rows
        _check_deal(y0, y1)
    _check_deal(np.zeros(MAX_CANDS, np.int64), np.full(MAX_CANDS, GROUP_H - 1))       # 1,024: four starts in every word
    _check_deal(np.array([15]), np.array([15]))


def test_entry_word_round_trip():
    x0, x1, cand = np.meshgrid(np.arange(64, dtype=np.uint64), np.arange(64, dtype=np.uint64), np.arange(64, dtype=np.uint64),
                               indexing="ij")
    for first, row0 in ((0, 0), (1, 15), (63, 7), (64, 8), (1008, 0), (MAX_TASKS - 1, 15)):
        w = _span_entry(np.uint64(first), np.uint64(row0), x0, x1, cand)
        assert (w < 2 ** 32).all()
        w = w.astype(np.uint32)
        assert ((w & 1023) == first).all() and (((w >> 10) & 15) == row0).all()
        assert (((w >> 14) & 63) == x0).all() and (((w >> 20) & 63) == x1).all() and ((w >> 26) == cand).all()


def _span_terms(rec, bx0, bx1):
    """span_terms: legacy_row_span's row-independent part, in float32; None: the rows keep the whole box."""
    ax, ay, v0x, v0y, v1x, v1y, d00, d01, d11, den = rec
    if not all(np.isfinite(x) for x in rec) or not abs(den) > 0:
        return None
    with np.errstate(all="ignore"):
        T = max(abs(f(f(f(bx0) + f(0.5)) - ax)), abs(f(f(f(bx1) + f(0.5)) - ax)))
        idn = f(f(1.0) / den)
        p0, p1 = f(abs(v0x) * T), f(abs(v1x) * T)
        av, kv = f(f(f(d11 * v0x) - f(d01 * v1x)) * idn), f(f(f(d11 * v0y) - f(d01 * v1y)) * idn)
        aw, kw = f(f(f(d00 * v1x) - f(d01 * v0x)) * idn), f(f(f(d00 * v1y) - f(d01 * v0y)) * idn)
    return idn, av, aw, kv, kw, p0, p1


def _span_row(terms, rec, py, bx0, bx1):
    """span_row: one row from the candidate's terms; of the record: ax, ay, v0y, v1y, d00, d01, d11."""
    import math
    if terms is None:
        return bx0, bx1
    idn, av, aw, kv, kw, p0, p1 = terms
    ax, ay, _, v0y, _, v1y, d00, d01, d11, _ = rec
    E = f(2.0 ** -18)
    with np.errstate(all="ignore"):
        Y = f(f(f(py) + f(0.5)) - ay)
        aY, aid = abs(Y), abs(idn)
        s0, s1 = f(p0 + f(abs(v0y) * aY)), f(p1 + f(abs(v1y) * aY))
        mv = f(aid * f(f(abs(d11) * s0) + f(abs(d01) * s1)))
        mw = f(aid * f(f(abs(d00) * s1) + f(abs(d01) * s0)))
        cv, cw = f(kv * Y), f(kw * Y)
        lo, hi = f(-1e30), f(1e30)
        for a, c, e in ((av, cv, f(E * mv)), (aw, cw, f(E * mw)),
                        (f(-f(av + aw)), f(f(1.0) - f(cv + cw)), f(E * f(f(1.0) + f(f(2.0) * f(mv + mw)))))):
            b = f(-e - c)
            if a > 0:
                lo = max(lo, f(b / a))
            elif a < 0:
                hi = min(hi, f(b / a))
            elif b > 0:
                lo, hi = f(1e30), f(-1e30)
        flo, fhi = f(f(lo + ax) - f(0.5)), f(f(hi + ax) - f(0.5))
        slo = f(f(2.0 ** -12) * f(f(abs(lo) + abs(ax)) + f(1.0)))
        shi = f(f(2.0 ** -12) * f(f(abs(hi) + abs(ax)) + f(1.0)))
        a, b = f(flo - slo), f(fhi + shi)
    a = 1e9 if np.isnan(a) else min(max(float(a), -1e9), 1e9)
    b = 1e9 if np.isnan(b) else min(max(float(b), -1e9), 1e9)
    return max(bx0, math.ceil(a)), min(bx1, math.floor(b))


def test_split_evaluation_gives_the_same_spans():
    """Per-candidate terms, then the per-row part: the spans of the one-piece restatement (legacy_span),
    over group-sized clips of small, large, sliver, hair-thin and pixel-centre-cornered triangles of both
    windings -- and, for a record that is not finite or has denom 0, the whole box."""
    rng = np.random.default_rng(0x5B11)
    n_rows = n_cut = 0
    for pts in _triangles(rng, 600):
        rec = _record(pts)
        for cx, cy in (pts.mean(0), pts[0]):
            gx0, gy0 = int(max(0.0, cx)) // GROUP_W * GROUP_W, int(max(0.0, cy)) // GROUP_H * GROUP_H
            bx0 = gx0 + int(rng.integers(0, GROUP_W))
            bx1 = int(rng.integers(bx0, gx0 + GROUP_W))
            terms = _span_terms(rec, bx0, bx1)      # once per candidate
            for py in range(gy0, gy0 + GROUP_H):
                got, want = _span_row(terms, rec, py, bx0, bx1), legacy_span(rec, py, bx0, bx1)
                assert got == want, f"row {py} of box [{bx0}, {bx1}]: {got} != {want} for {pts.tolist()}"
                n_rows += 1
                n_cut += want != (bx0, bx1)
    assert n_rows > 15000 and n_cut > n_rows // 4
    good = _record(np.array([[3.5, 2.5], [40.25, 4.0], [9.0, 14.5]], f))
    for k, bad in [(k, v) for k in range(10) for v in (f(np.inf), f(np.nan))] + [(9, f(0.0))]:
        rec = tuple(bad if i == k else x for i, x in enumerate(good))
        assert _span_terms(rec, 2, 50) is None
        assert _span_row(None, rec, 7, 2, 50) == legacy_span(rec, 7, 2, 50) == (2, 50)
