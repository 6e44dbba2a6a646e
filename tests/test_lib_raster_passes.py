"""The seams between k_lib_raster's phases (lib_raster_tile: gather, list write-out, deep passes or
select / stage / box pairs, finish), which the other scenes cross only incidentally: one raster tile whose
candidate list is one entry either side of LIB_CHUNK (128: one staging pass, no sort | sorted, several
passes), LIB_CAND_SHALLOW (256: the shallow raster after the first frame | the deep one again) and
LIB_CAND_DEEP (1024: one candidate round | two).

Scene: a 64x32 frame (two bin tiles, eight raster tiles), identity view-projection, no culling.  n small
triangles (3-8 px wide, 3-5.4 px high) whose boxes all lie inside the 32x8 raster tile at x 0..31, rows
8..15 counted from either edge -- on two exact depth planes (z ties, decided by submission order) plus
scattered depths -- and one triangle over the whole tile, submitted last and nearest: after the pass that
holds it, every other candidate is rejected by the tile's largest key z or by its own pixels' keys.  The
tile's list holds n + 1 entries.  A pass of at most SCAN_MAX input triangles keeps no bins -- every primitive
is a candidate of every busy tile, and max_tile_bin reads 0 -- so each size also runs with PAD zero-area
triangles submitted first: the setup drops them, but they count as input, the pass bins, and the tile's bin
holds exactly n + 1.  Results: the oracle's, depth bit for bit."""
import functools

import numpy as np
import pytest

from helpers import assert_depth_bitexact, assert_float_close
from test_sorted_lists import _render_check

W, H = 64, 32
SIZES = [1, 127, 128, 129, 255, 256, 257, 1023, 1024, 1025]
COVER_Z = -0.95
SCAN_MAX, PAD = 512, 600   # shs_lib_plan.hpp SCAN_MAX_PRIMS; PAD > SCAN_MAX: bins at every size
# the light camera's margins are in world units: the casters are the NDC-sized soup scaled up, lit almost
# along z -- the cover nearest the light (it hides the rest), then farthest (the small triangles show)
SUNS = [(0.02, -0.03, 1.0), (0.02, -0.03, -1.0)]
CASTER_SCALE = 400.0


def _ndc(px, py):
    return np.stack([2.0 * px / (W - 1) - 1.0, 2.0 * py / (H - 1) - 1.0], axis=-1)   # screen = (ndc / 2 + 0.5) * (size - 1)


@functools.lru_cache(maxsize=None)
def _soup(n, cover=True, pad=0):
    """(positions, normals, pixel-space xy [n, 3, 2] of the small triangles)."""
    rng = np.random.default_rng(1000 + n)
    cx, cy = rng.uniform(6.0, 26.0, n), rng.uniform(11.8, 12.2, n)
    a, b = rng.uniform(1.8, 3.7, n), rng.uniform(1.75, 2.5, n)         # half width, half height
    j = rng.uniform(-0.3, 0.3, (n, 3, 2)) * (1.0, 2.0 / 3.0)
    xy = np.stack([np.stack([cx - a, cy - b], -1), np.stack([cx + a, cy - b], -1), np.stack([cx, cy + b], -1)], 1) + j
    z = np.float32([0.0, 0.5])[rng.integers(0, 2, n)]
    z = np.where(rng.random(n) < 0.3, rng.uniform(-0.9, 0.9, n).astype(np.float32), z)
    zc = np.repeat(z[:, None, None], 3, axis=1)
    zc = zc + np.where((rng.random(n) < 0.15)[:, None, None], rng.normal(scale=0.02, size=(n, 3, 1)), 0.0)   # some tilted
    pos = np.concatenate([_ndc(xy[..., 0], xy[..., 1]), zc], axis=2)
    if cover:   # symmetric about the frame's middle: it covers x 0..31 of rows 8..22, whichever way the rows are counted
        cxy = np.array([[0.1, 0.2], [0.1, 30.8], [62.9, 15.5]])
        pos = np.concatenate([pos, np.concatenate([_ndc(cxy[:, 0], cxy[:, 1]), np.full((3, 1), COVER_Z)], axis=1)[None]], axis=0)
    pos = np.concatenate([np.zeros((pad, 3, 3)), pos], axis=0).reshape(-1, 3).astype(np.float32)
    nrm = rng.normal(size=pos.shape).astype(np.float32)   # distinct shading per triangle: the winner shows
    return pos, nrm, xy


def _draw(n, cover=True, pad=0):
    from shs_gpu.lib_path import LibDraw, LibMesh
    pos, nrm, _ = _soup(n, cover, pad)
    return LibDraw(mesh=LibMesh(pos, nrm), program=2, cull_mode=0)


def _frame(depth=True):
    from shs_gpu.lib_path import LibFrame
    return LibFrame(W, H, depth_motion=depth, zn=1.0, zf=1.0, bg_gradient=False, clear_hdr=(0.1, 0.2, 0.3, 1.0))


@functools.lru_cache(maxsize=None)
def _painter_ref(oracle_mod, n, cover, pad):
    return oracle_mod.pbr_forward(_frame(False), [_draw(n, cover, pad)], None)[0]


@functools.lru_cache(maxsize=None)
def _caster(n, pad):
    d = _draw(n, pad=pad)
    d.model = (np.eye(4, dtype=np.float32) * np.float32([CASTER_SCALE, CASTER_SCALE, CASTER_SCALE, 1.0])).reshape(16)
    return d


@functools.lru_cache(maxsize=None)
def _shadow_ref(oracle_mod, n, sun, pad):
    return oracle_mod.shadow_map((W, H), sun, [_caster(n, pad)])


@pytest.mark.parametrize("n", SIZES)
def test_scene_stays_in_one_raster_tile_and_keeps_every_triangle(oracle_mod, n):
    """The builders, on the CPU: every small triangle's pixel box inside the tile, none dropped by the
    setup (so the tile's list holds n + 1 entries), the cover in front of every pixel of the tile."""
    _, _, xy = _soup(n)
    assert xy[..., 0].min() > 1.0 and xy[..., 0].max() < 31.0
    assert xy[..., 1].min() > 9.0 and xy[..., 1].max() < 15.0     # rows 8..15 from either edge: one tile row
    assert (xy[..., 0].max(1) - xy[..., 0].min(1)).min() >= 3.0 and (xy[..., 0].max(1) - xy[..., 0].min(1)).max() <= 8.0
    assert (xy[..., 1].max(1) - xy[..., 1].min(1)).min() >= 3.0
    _, rd, _, rst = oracle_mod.pbr_forward(_frame(), [_draw(n)], None)
    assert rst["tri_input"] == rst["tri_after_clip"] == rst["tri_raster"] == n + 1
    _, rdp, _, rstp = oracle_mod.pbr_forward(_frame(), [_draw(n, pad=PAD)], None)
    assert rstp["tri_input"] == n + 1 + PAD and rstp["tri_raster"] == n + 1 and np.array_equal(rdp, rd)
    assert (np.abs(rd[8:16, 0:32] - (COVER_Z * 0.5 + 0.5)) < 1e-6).all() and (rd == np.float32(1.0)).any()
    # without the cover the small triangles show, tie planes included
    _, rd0, _, rst0 = oracle_mod.pbr_forward(_frame(), [_draw(n, False)], None)
    assert rst0["tri_raster"] == n and (rd0 != np.float32(1.0)).sum() >= 4


@pytest.mark.gpu
@pytest.mark.parametrize("pad", [0, PAD])
@pytest.mark.parametrize("n", SIZES)
def test_camera_frames_deep_then_shallow(oracle_mod, n, pad):
    """A fresh context's first camera pass runs the deep raster; the second the shallow one when the
    fullest bin (without bins: the input) held <= 256 entries, the deep one again otherwise."""
    import shs_gpu
    binned = n + 1 + pad > SCAN_MAX
    with shs_gpu.Context(0) as ctx:
        for _ in range(2):
            st, _ = _render_check(ctx, oracle_mod, _frame(), [_draw(n, pad=pad)])
            assert st["max_tile_bin"] == (n + 1 if binned else 0), st["max_tile_bin"]
            assert st["tri_input"] == n + 1 + pad and st["tri_raster"] == n + 1


@pytest.mark.gpu
@pytest.mark.parametrize("cover,pad", [(True, 0), (False, 0), (True, PAD)])
@pytest.mark.parametrize("n", SIZES)
def test_painters_order(oracle_mod, n, cover, pad):
    """No depth target: every fragment writes and the last submitted wins -- unsorted multi-pass staging,
    inverted-sequence keys, no depth bound may reject anything."""
    import shs_gpu
    rh = _painter_ref(oracle_mod, n, cover, pad)
    with shs_gpu.Context(0) as ctx:
        for _ in range(2):
            ctx.render_pbr_forward(_frame(False), [_draw(n, cover, pad)])
            gh, _, _ = ctx.resolve_lib()
            assert_float_close(gh, rh, what="hdr")


@pytest.mark.gpu
@pytest.mark.parametrize("sun,pad", [(SUNS[0], 0), (SUNS[0], PAD), (SUNS[1], PAD)])
@pytest.mark.parametrize("n", SIZES)
def test_shadow_pass_twice(oracle_mod, n, sun, pad):
    """The same triangles as shadow casters into a 64x32 map: the deep, then the predicted shadow raster."""
    import shs_gpu
    sm_ref, lvp_ref = _shadow_ref(oracle_mod, n, sun, pad)
    assert (sm_ref != np.float32(1.0)).sum() > 500
    with shs_gpu.Context(0) as ctx:
        for _ in range(2):
            lvp = ctx.render_shadow_map((W, H), sun, [_caster(n, pad)])
            assert np.array_equal(lvp.view(np.uint32), lvp_ref.view(np.uint32)), "light camera differs"
            assert_depth_bitexact(ctx.resolve_shadow_map(), sm_ref)


@pytest.mark.gpu
def test_split_tile_parts(oracle_mod):
    """The tile's 258 entries as parts of at most 64 (k_lib_plan): merged keys, written by the last part."""
    import shs_gpu
    with shs_gpu.Context(0) as ctx:
        ctx.set_lib_part(64)
        for _ in range(2):
            st, _ = _render_check(ctx, oracle_mod, _frame(), [_draw(257, pad=PAD)])   # (parts need bins)
            assert st["max_tile_bin"] == 258
