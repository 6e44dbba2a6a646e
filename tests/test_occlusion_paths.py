"""Software occlusion pass on crafted scenes: the paths of csrc/shs_occlusion.hip and csrc/shs_abi_occ.cpp
that tests/test_occlusion.py's random boxes and spheres do not reach, each against oracle.occlusion_pass
bit-exactly (occluded flags, the visible list in visit order, the depth bits; no tolerances):

1. meshes of more than one 1024-triangle chunk, the deciding triangles in the last chunk;
2. a buffer over 2^22 pixels (chunk = 511: idle lanes, a slot across 64 pair windows);
3. the pair-window layout at its edges (slot / window boundaries, a full start word, 1024 slots, skips);
4. every round of the rect test (a one-pixel hole in a full-screen occluder);
5. the compare z_near <= depth + eps at equality and one ulp past it;
6. the host's visit order (ties, +-0 keys, duplicates, out-of-range indices, n = 0 .. 3, invalid rects);
7. one context through a sequence of these;  8. shared meshes, a model with a free bottom row, an
   index >= n_verts;  9. the buffer size limit.

Most scenes are pixel-exact: view_proj is the identity (or flips z), models are the identity, the buffer
sides are powers of two and a vertex at pixel (px, py) sits at (2 px / W - 1, 2 py / H - 1, z), so sx, sy
are exact and a triangle with integer corners a .. b has a clamped box of b - a + 1 columns.  Every
triangle of a crafted mesh has its own z: a (triangle, pixel) pair given to the wrong slot changes the
depth image.  Expected depths always come from the oracle, never from z (the interpolation may be an ulp
off the plane).

Each scene has a CPU test (no marker) that runs the oracle alone and asserts what the scene is for: the
chunk count (`_chunk`), the per-chunk pair totals and the property of the
window layout it hits (from `_tri_counts`, a numpy float32 restatement of the per-triangle setup, and
`stored_order`, the mesh upload's triangle order), and that both outcomes occur where the case needs them.
A mesh of more than 256 triangles is stored in Morton order of its centroids (tests/test_spatial_order.py);
the chunk scenes place their groups in the centroid bounds' octants so that the stored order is known."""
import functools

import numpy as np
import pytest

from test_spatial_order import stored_order

OCC_WIN = 131072          # pairs per window (csrc/shs_occlusion.hip OCC_WIN)
F = np.float32


def _diag(*d):
    return np.diag(np.asarray(d, F)).reshape(-1)


IDENT = _diag(1, 1, 1, 1)
ZFLIP = _diag(1, 1, -1, 1)      # nz = -z: a larger model z is nearer (and later in the stored order)
# clip = (x, y, z - 1, z): w = z, nz = 1 - 1 / z; z <= 0.001 fails the clip.w test, z < 0.5 the nz test
PERSP = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 1, 0, 0, -1, 0], F)


def _chunk(W, H):
    """Triangles per raster chunk (csrc/shs_abi_occ.cpp): a chunk's pair total leaves room for one window
    below 2^32.  For every buffer of this file that is min(1024, 0xffffffff // (W * H))."""
    chunk = min(1024, (2 ** 32 - OCC_WIN) // (W * H))
    assert chunk == min(1024, 0xFFFFFFFF // (W * H))
    return chunk


def _mesh(W, H, px, z, idx=None):
    """px [n, 3, 2] pixel coordinates and z [n] or [n, 3] -> a LibMesh of n triangles (3 n own vertices)."""
    from shs_gpu.lib_path import LibMesh
    px = np.asarray(px, np.float64).reshape(-1, 3, 2)
    z = np.asarray(z, np.float64)
    z = np.repeat(z[:, None], 3, 1) if z.ndim == 1 else z
    pos = np.stack([2.0 * px[..., 0] / W - 1.0, 2.0 * px[..., 1] / H - 1.0, z], -1).reshape(-1, 3).astype(F)
    return LibMesh(positions=pos, indices=np.arange(len(pos), dtype=np.uint32) if idx is None else np.asarray(idx, np.uint32))


def _box(x0, y0, w, h):
    """A triangle whose clamped box is the w x h pixels at (x0, y0); w, h >= 2, inside the buffer."""
    return [(x0, y0), (x0 + w - 1, y0), (x0, y0 + h - 1)]


def _corner(W, H, w, h):
    """A triangle whose box is clamped by the buffer's far corner to w x h pixels (w, h >= 1)."""
    return [(W - w, H - h), (W, H - h), (W - w, H)]


def _rect(x0, y0, x1, y1):
    """Two triangles over the pixel-aligned rectangle [x0, x1] x [y0, y1] (covers pixels x0 .. x1 - 1)."""
    return [[(x0, y0), (x1, y0), (x1, y1)], [(x0, y0), (x1, y1), (x0, y1)]]


def _aabb(W, H, x0, y0, x1, y1, z0, z1):
    """World AABB whose corners sit at the pixel corners (x0, y0) .. (x1, y1): its screen rect is the
    pixels x0 .. min(x1, W - 1) by y0 .. min(y1, H - 1) under IDENT / ZFLIP."""
    return (np.array([2.0 * x0 / W - 1.0, 2.0 * y0 / H - 1.0, min(z0, z1)], F),
            np.array([2.0 * x1 / W - 1.0, 2.0 * y1 / H - 1.0, max(z0, z1)], F))


def _m4v(m, v):
    m = np.asarray(m, F)
    return np.stack([(m[r] * v[:, 0] + m[4 + r] * v[:, 1]) + (m[8 + r] * v[:, 2] + m[12 + r] * v[:, 3]) for r in range(4)], 1)


LIVE, SKIP_INDEX, SKIP_W, SKIP_NZ, SKIP_AREA, SKIP_BOX = range(6)


def _tri_counts(mesh, model, vp, W, H):
    """float32 restatement of rasterize_mesh_depth_transformed's per-triangle setup -> (pairs per triangle
    = clamped box area or 0, skip reason), in MeshData order."""
    pos = np.asarray(mesh.positions, F)
    idx = np.asarray(mesh.indices, np.int64).reshape(-1, 3)
    reason = np.full(len(idx), LIVE)
    bad = (idx >= len(pos)).any(1)
    i = np.where(idx < len(pos), idx, 0)
    with np.errstate(all="ignore"):
        wp = _m4v(model, np.c_[pos, np.ones(len(pos), F)])
        wp[:, 3] = 1.0
        clip = _m4v(vp, wp)
        w_bad = clip[:, 3] <= F(0.001)
        nd = clip[:, :3] / np.where(w_bad, F(1), clip[:, 3])[:, None]
        nz_bad = (nd[:, 2] < F(-1)) | (nd[:, 2] > F(1))
        sx = (nd[:, 0] + F(1)) * F(0.5) * F(W)
        sy = (nd[:, 1] + F(1)) * F(0.5) * F(H)
    X, Y = sx[i], sy[i]
    area = (X[:, 2] - X[:, 0]) * (Y[:, 1] - Y[:, 0]) - (Y[:, 2] - Y[:, 0]) * (X[:, 1] - X[:, 0])
    x0 = np.maximum(0, np.floor(X.min(1)).astype(np.int64))
    y0 = np.maximum(0, np.floor(Y.min(1)).astype(np.int64))
    x1 = np.minimum(W - 1, np.ceil(X.max(1)).astype(np.int64))
    y1 = np.minimum(H - 1, np.ceil(Y.max(1)).astype(np.int64))
    for code, mask in ((SKIP_BOX, (x0 > x1) | (y0 > y1)), (SKIP_AREA, np.abs(area) <= F(1e-6)),
                       (SKIP_NZ, nz_bad[i].any(1)), (SKIP_W, w_bad[i].any(1)), (SKIP_INDEX, bad)):
        reason[mask] = code          # the reference's first failing test wins: applied last
    cnt = np.where(reason == LIVE, (x1 - x0 + 1) * (y1 - y0 + 1), 0)
    return cnt, reason


def _stored(mesh):
    n = mesh.indices.size // 3
    return stored_order(mesh.positions, mesh.indices) if n > 256 else np.arange(n)


def _chunks(cnt_stored, chunk):
    return [cnt_stored[c:c + chunk] for c in range(0, len(cnt_stored), chunk)]


def _starts(cnt):
    """First pair of each live slot of one chunk (compacted) and the chunk's pair total."""
    live = cnt[cnt > 0]
    return np.concatenate([[0], np.cumsum(live)[:-1]]) if len(live) else np.zeros(0, np.int64), int(live.sum())


def _scene(W, H, objs, fv=None, view=IDENT, vp=IDENT, eps=1e-4):
    return dict(W=W, H=H, objs=objs, fv=np.arange(len(objs), dtype=np.uint32) if fv is None else np.asarray(fv, np.uint32),
                view=view, vp=vp, eps=eps)


@functools.lru_cache(maxsize=None)
def _oracle():
    from oracle import oracle
    oracle.lib()
    return oracle


def _want(s, **kw):
    """The oracle's result, computed once per scene and shared (never modified)."""
    if "want" not in s or kw:
        r = _oracle().occlusion_pass(s["W"], s["H"], s["view"], s["vp"], s["objs"], s["fv"], depth_epsilon=s["eps"], **kw)
        if kw:
            return r
        s["want"] = r
    return s["want"]


def _same(got, want, what=""):
    assert np.array_equal(got[0], want[0]), f"{what}: occluded flags differ at {np.nonzero(got[0] != want[0])[0][:8]}"
    assert np.array_equal(got[1], want[1]), f"{what}: visible lists differ: {got[1][:12]} vs {want[1][:12]}"
    g, w = got[2].view(np.uint32), want[2].view(np.uint32)
    assert np.array_equal(g, w), f"{what}: {int((g != w).sum())} depth values differ, first at (y, x) {np.argwhere(g != w)[:4].tolist()}"


def _gpu(ctx, s, **kw):
    return ctx.occlusion_pass(s["W"], s["H"], s["view"], s["vp"], s["objs"], s["fv"], depth_epsilon=s["eps"], **kw)


def _check_gpu(s, what=""):
    import shs_gpu
    want = _want(s)
    with shs_gpu.Context(0) as ctx:
        got = _gpu(ctx, s)
    _same(got, want, what)


# ---- 1. more triangles than a chunk -------------------------------------------------------------------
CHUNK_SIZES = [1024, 1025, 2048, 2 * 1024 + 37]


@functools.lru_cache(maxsize=None)
def _chunk_scene(n_tris):
    """256 x 128, ZFLIP.  Object 0's mesh, in stored order: group A, fillers (3 x 3 boxes all over the
    buffer, far, z in the lower half of the centroid bounds); with 2085 triangles group B, 1024 degenerate
    triangles (z upper half, y lower half: a whole middle chunk of no pairs); group C (z upper half, y upper
    half), which ends the stored order: small triangles and the one near triangle that covers the probes'
    rect.  Then: P, hidden by that triangle alone; Q, object 0's mesh again (nearer by its model) behind
    the same rect: occluded, its prefetched chunk 0 dropped; Z, small and visible; M2, the mesh a third time,
    shifted and visible."""
    W, H = 256, 128
    rng = np.random.default_rng(n_tris)
    mid = n_tris == 2 * 1024 + 37
    n_c = n_tris - 2048 if mid else 1
    n_b = 1024 if mid else 0
    n_a = n_tris - n_b - n_c
    px, z = [], []
    xs, ys = rng.integers(0, W - 3, n_a), rng.integers(0, H - 3, n_a)
    ys[:2] = (0, H - 4)                                     # the centroid bounds' y span
    for k in range(n_a):
        px.append(_box(xs[k], ys[k], 3, 3))
        z.append(-0.9 + 0.8 * k / n_a)
    for k in range(n_b):                                    # two identical corners: area 0
        x, y = rng.integers(0, W), rng.integers(0, 30)
        px.append([(x, y), (x, y), (x + 5, y + 3)])
        z.append(0.2 + 0.3 * k / n_b)
    for k in range(n_c - 1):
        px.append(_box(rng.integers(0, W - 4), rng.integers(100, 120), 4, 3))
        z.append(0.5 + 0.3 * k / n_c)
    px.append([(0, 96), (W, 96), (W, H)])                   # the near triangle: covers y <= 96 + x / 8
    z.append(0.9)
    mesh = _mesh(W, H, px, z)
    tiny = _mesh(W, H, [_box(5, 5, 4, 4)], [0.95])
    zq = _mesh(W, H, _rect(10, 10, 21, 21), [0.31, 0.32])
    full = _aabb(W, H, 0, 0, W, H, 0.9, 1.0)
    probe = (200, 98, 250, 108)
    shift = IDENT.copy()
    shift[12:15] = (2.0 * 2 / W, 0.0, 0.05)                 # 2 pixels right, 0.05 nearer
    shift2 = IDENT.copy()
    shift2[12:15] = (2.0 * -3 / W, 2.0 * 1 / H, -0.03)
    objs = [(mesh, IDENT, *full),
            (tiny, IDENT, *_aabb(W, H, *probe, 0.4, 0.5)),
            (mesh, shift, *_aabb(W, H, *probe, 0.3, 0.35)),
            (zq, IDENT, *_aabb(W, H, 10, 10, 20, 20, 0.2, 0.3)),
            (mesh, shift2, *_aabb(W, H, 0, 0, W, H, 0.0, 0.1))]
    s = _scene(W, H, objs, fv=[3, 2, 4, 0, 1], view=ZFLIP, vp=ZFLIP)
    s.update(mesh=mesh, near=n_tris - 1, probe=probe)
    return s


@pytest.mark.parametrize("n_tris", CHUNK_SIZES)
def test_chunk_scene_preconditions(oracle_mod, n_tris):
    s = _chunk_scene(n_tris)
    W, H, mesh = s["W"], s["H"], s["mesh"]
    chunk = _chunk(W, H)
    assert chunk == 1024 and mesh.indices.size == 3 * n_tris
    cnt, reason = _tri_counts(mesh, IDENT, s["vp"], W, H)
    order = _stored(mesh)
    per = _chunks(cnt[order], chunk)
    assert len(per) == (n_tris + 1023) // 1024
    totals = [int(c.sum()) for c in per]
    assert totals[0] > 0 and totals[-1] > 0 and max(totals) < OCC_WIN
    if n_tris == 2 * 1024 + 37:
        assert totals[1] == 0 and (reason[order][1024:2048] == SKIP_AREA).all()   # a whole chunk of skips
        assert len(per[-1]) == 37
    # the near triangle sits in the last chunk (and, the 1024 case apart, not in the first)
    at = int(np.nonzero(order == s["near"])[0][0])
    assert at // chunk == len(per) - 1 and cnt[s["near"]] == W * (H - 96)
    occ, vis, depth = _want(s)
    assert vis.tolist() == [0, 3, 4] and occ.tolist() == [0, 1, 1, 0, 0]
    # P and Q are hidden by the near triangle alone: without it (its pairs are the last chunk's) both
    # are visible, so a walk that drops or misindexes a later chunk flips their flags
    x0, y0, x1, y1 = s["probe"]
    near_z = F(0.05)
    assert np.abs(depth[y0:y1 + 1, x0:x1 + 1] - near_z).max() < 1e-6
    keep = np.delete(np.arange(n_tris), s["near"])
    from shs_gpu.lib_path import LibMesh
    cut = LibMesh(positions=mesh.positions, indices=mesh.indices.reshape(-1, 3)[keep].reshape(-1))
    objs = [(cut if o[0] is mesh else o[0], *o[1:]) for o in s["objs"]]
    occ2, _, _ = _oracle().occlusion_pass(W, H, s["view"], s["vp"], objs, s["fv"])
    assert occ2.tolist() == [0, 0, 0, 0, 0]


@pytest.mark.gpu
@pytest.mark.parametrize("n_tris", CHUNK_SIZES)
def test_chunk_scene_exact(oracle_mod, n_tris):
    _check_gpu(_chunk_scene(n_tris), f"{n_tris} triangles")


# ---- 2. chunk < 1024 ----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _big_buffer_scene():
    """4096 x 2049: chunk = 511.  A 1536-triangle sphere, small on screen (4 chunks, the last of 3
    triangles); a mesh whose one chunk holds a full-screen triangle pair between small triangles (a slot
    across 64 windows, slots before and after it); an object behind the pair (occluded only if every window
    of both slots was rastered); a near small object; the sphere again, behind the pair."""
    from shs_gpu import scene_lib
    W, H = 4096, 2049
    sph = scene_lib.sphere_mesh(seg=32, rings=24)
    m0 = IDENT.copy()
    m0[0], m0[5], m0[10] = 0.1, 0.1, 0.1
    m0[12:15] = (-0.5, 0.3, -0.5)
    m4 = m0.copy()
    m4[12:15] = (0.2, -0.2, 0.5)
    px = [_box(100, 200, 10, 10), [(0, 0), (W, 0), (W, H)], _box(3000, 1000, 7, 9), [(0, 0), (W, H), (0, H)],
          _box(2000, 40, 12, 5)]
    pair = _mesh(W, H, px, [0.0, 0.2, 0.05, 0.21, 0.1])
    small = _mesh(W, H, _rect(700, 700, 741, 731), [-0.8, -0.81])
    objs = [(sph, m0, *scene_lib.world_aabb(sph, m0)),
            (pair, IDENT, *_aabb(W, H, 0, 0, W, H, 0.1, 0.2)),
            (small, IDENT, *_aabb(W, H, 100, 100, 4000, 1900, 0.5, 0.6)),
            (small, IDENT, *_aabb(W, H, 700, 700, 740, 730, -0.8, -0.7)),
            (sph, m4, *scene_lib.world_aabb(sph, m4))]
    s = _scene(W, H, objs, fv=[4, 3, 2, 1, 0])
    s.update(sph=sph, m0=m0, pair=pair)
    return s


def test_big_buffer_scene_preconditions(oracle_mod):
    s = _big_buffer_scene()
    W, H = s["W"], s["H"]
    chunk = _chunk(W, H)
    assert W * H == 8392704 and chunk == 511 and len(s["objs"]) <= 8
    cnt, _ = _tri_counts(s["sph"], s["m0"], IDENT, W, H)
    per = _chunks(cnt[_stored(s["sph"])], chunk)
    assert [len(c) for c in per] == [511, 511, 511, 3] and all(c.sum() > 0 for c in per[:3])
    assert cnt.max() < 200 * 200                            # small on screen
    cnt, _ = _tri_counts(s["pair"], IDENT, IDENT, W, H)
    # (2049 is no power of two: sy is rounded, so the small boxes may gain a row)
    assert cnt[[1, 3]].tolist() == [W * H, W * H] and ((cnt[[0, 2, 4]] >= 60) & (cnt[[0, 2, 4]] <= 130)).all()
    start, total = _starts(cnt)
    assert total < 2 ** 32
    # each full-screen slot runs across 64 windows and more, with slots before and after it in the chunk
    for k in (1, 3):
        a, e = start[k], start[k] + cnt[k]
        assert (e - 1) // OCC_WIN - a // OCC_WIN + 1 >= 64 and a > 0 and e < total
    occ, vis, depth = _want(s)
    assert occ.tolist() == [0, 0, 1, 0, 1] and vis.tolist() == [3, 0, 1]
    assert (depth < 1.0).all()


@pytest.mark.gpu
def test_big_buffer_scene_exact(oracle_mod):
    _check_gpu(_big_buffer_scene())


# ---- 3. the window layout at its edges ----------------------------------------------------------------
WINDOW_CASES = ["a_slot_ends_on_edge", "b_straddle_by_one", "c_three_whole_windows", "d_total_multiple_of_window",
                "d_total_multiple_of_word", "e_full_start_word", "f_1024_slots", "g_skips_interleaved"]


@functools.lru_cache(maxsize=None)
def _window_scene(case):
    """1024 x 512 (4 windows of pairs per full-screen box), one crafted chunk as object 0's mesh."""
    W, H = 1024, 512
    rng = np.random.default_rng(len(case))
    vp = IDENT
    extra = []
    if case == "g_skips_interleaved":
        return _skip_scene()
    if case == "a_slot_ends_on_edge":
        tris = [_box(0, 0, 512, 256), _box(300, 200, 512, 256), _box(900, 17, 7, 5)]
    elif case == "b_straddle_by_one":
        tris = [_box(3, 5, 510, 257), _corner(W, H, 1, 1), _corner(W, H, 2, 1), _box(600, 300, 30, 20)]
    elif case == "c_three_whole_windows":
        tris = [_box(50, 60, 10, 10), _box(0, 0, 1024, 512), _box(700, 400, 9, 9)]
        # behind the big triangle (it covers x / 1023 + y / 511 <= 1): hidden only if all its windows ran
        extra = [(_mesh(W, H, [_box(1, 1, 5, 5)], [-0.95]), IDENT, *_aabb(W, H, 2, 2, 400, 250, 0.95, 0.99))]
    elif case == "d_total_multiple_of_window":
        tris = [_box(10, 10, 256, 256), _box(400, 100, 512, 256), _box(700, 250, 256, 256)]
    elif case == "d_total_multiple_of_word":
        tris = [_box(100, 100, 512, 256), _box(40, 50, 8, 8)]
    elif case == "e_full_start_word":
        tris = [_box(20, 30, 8, 8)] + [_corner(W, H, 1, 1)] * 64 + [_box(500, 300, 5, 5)]
    elif case == "f_1024_slots":
        tris = [_box(3 + 31 * (k % 32) + int(rng.integers(0, 20)), 2 + 15 * (k // 32) + int(rng.integers(0, 8)), 2, 2)
                for k in range(1024)]
    # an own z per triangle, the larger boxes farther so that every slot shows in the image; the one-pair
    # triangles of (e) all hit the corner pixel: the nearest is in the middle of their word
    cnt = np.array([(max(p[0] for p in t) - min(p[0] for p in t) + 1) * (max(p[1] for p in t) - min(p[1] for p in t) + 1)
                    for t in tris])
    rank = np.argsort(np.argsort(-cnt, kind="stable"), kind="stable")
    z = 0.9 - 1.7 * (rank + 1) / (len(tris) + 1)
    if case == "e_full_start_word":
        z[1:65] = -0.5 - 0.005 * np.r_[np.arange(37), 37 - np.arange(27) * 0.5]   # minimum at the 37th
    mesh = _mesh(W, H, tris, z)
    s = _scene(W, H, [(mesh, IDENT, *_aabb(W, H, 0, 0, W, H, -1.0, -0.98))] + extra, vp=vp)
    s.update(mesh=mesh)
    return s


@functools.lru_cache(maxsize=None)
def _skip_scene():
    """(g) 1024 x 512 under PERSP: live triangles (corners on pixel centres, so their boxes survive the
    rounding of x / w) interleaved with skipped ones, one per reason in turn: slot != thread index."""
    W, H = 1024, 512
    rng = np.random.default_rng(5)
    pos = []
    for k in range(120):
        zv = 1.0 + rng.uniform(0.0, 1.0)                    # nz = 1 - 1 / z in [0, 0.5]
        x0, y0 = rng.integers(0, W - 80), rng.integers(0, H - 60)
        w, h = rng.integers(3, 70), rng.integers(3, 50)
        t = np.array([(x0 + 0.5, y0 + 0.5), (x0 + w - 1.5, y0 + 0.5), (x0 + 0.5, y0 + h - 1.5)])
        zs = np.full(3, zv)
        if k % 2 == 1 or k % 16 == 0:                       # skipped: also two live ones in a row
            why = (k // 2) % 6
            if why == 0:
                t[1] = t[0]                                 # area 0
            elif why == 1:
                zs[rng.integers(0, 3)] = 0.0005             # clip.w <= 0.001
            elif why == 2:
                zs[rng.integers(0, 3)] = -1.0               # behind the camera
            elif why == 3:
                zs[rng.integers(0, 3)] = 0.4                # nz = -1.5
            elif why == 4:
                t[:, 0] += 3 * W                            # box off screen to the right
            else:
                t[:, 1] -= 2 * H                            # box above the screen
        nd = np.stack([2.0 * t[:, 0] / W - 1.0, 2.0 * t[:, 1] / H - 1.0], 1)
        pos.append(np.c_[nd * zs[:, None], zs])
    from shs_gpu.lib_path import LibMesh
    pos = np.concatenate(pos).astype(F)
    mesh = LibMesh(positions=pos, indices=np.arange(len(pos), dtype=np.uint32))
    mn, mx = np.array([-1, -1, 1], F), np.array([1, 1, 1], F)
    s = _scene(W, H, [(mesh, IDENT, mn, mx)], vp=PERSP)
    s.update(mesh=mesh)
    return s


@pytest.mark.parametrize("case", WINDOW_CASES)
def test_window_scene_preconditions(oracle_mod, case):
    s = _window_scene(case)
    W, H, mesh = s["W"], s["H"], s["mesh"]
    assert _chunk(W, H) == 1024 and mesh.indices.size // 3 <= 1024          # one chunk
    cnt, reason = _tri_counts(mesh, IDENT, s["vp"], W, H)
    cnt = cnt[_stored(mesh)]
    start, total = _starts(cnt)
    live = cnt[cnt > 0]
    end = start + live
    if case == "a_slot_ends_on_edge":
        assert end[0] == OCC_WIN and start[1] == OCC_WIN
    elif case == "b_straddle_by_one":
        assert live.tolist() == [510 * 257, 1, 2, 600] and start[2] == OCC_WIN - 1 and end[2] == OCC_WIN + 1
    elif case == "c_three_whole_windows":
        assert start[1] == 100 and live[1] == W * H and end[1] > 4 * OCC_WIN
        assert _want(s)[0].tolist() == [0, 1]
    elif case == "d_total_multiple_of_window":
        assert total == 2 * OCC_WIN and start[1] < OCC_WIN < end[1]
    elif case == "d_total_multiple_of_word":
        assert total % 64 == 0 and total % OCC_WIN == 64
    elif case == "e_full_start_word":
        assert start[1:65].tolist() == list(range(64, 128)) and (live[1:65] == 1).all()
        # all 64 cover the corner pixel; the nearest (z = -0.685) is the 38th of the word
        zs = mesh.positions[3::3, 2][:64]
        assert int(np.argmin(zs)) == 37 and abs(_want(s)[2][H - 1, W - 1] - (zs[37] * 0.5 + 0.5)) < 1e-6
    elif case == "f_1024_slots":
        assert len(live) == 1024 and (live == 4).all()
    else:
        assert set(reason.tolist()) == {LIVE, SKIP_W, SKIP_NZ, SKIP_AREA, SKIP_BOX}
        slot = np.cumsum(cnt > 0) - 1
        assert (slot[cnt > 0] != np.nonzero(cnt > 0)[0]).sum() > 40 and 40 < len(live) < 80
        assert total < OCC_WIN
    depth = _want(s)[2]
    assert (depth < 1.0).sum() > 0 and _want(s)[0][0] == 0
    # the triangles show with their own depths (a slot whose pairs go to another triangle changes the
    # image): all 1024 of (f), each at its one covered pixel, and at least three planes elsewhere
    if case == "f_1024_slots":
        assert (depth < 1.0).sum() == 1024 and len(np.unique(depth[depth < 1.0])) == 1024
    elif case not in ("e_full_start_word", "g_skips_interleaved"):
        assert len(np.unique(depth[depth < 1.0].round(4))) >= min(len(live), 3)


@pytest.mark.gpu
@pytest.mark.parametrize("case", WINDOW_CASES)
def test_window_scene_exact(oracle_mod, case):
    _check_gpu(_window_scene(case), case)


# ---- 4. rect test rounds ------------------------------------------------------------------------------
HOLES = [0, 1023, 1024, 8191, 8192, 8193, 65536, 300 * 225 - 1, None]


@functools.lru_cache(maxsize=None)
def _hole_scene(hole):
    """300 x 225.  Object 0: a sheet of four pixel-aligned rectangles around the one-pixel hole at rect
    index `hole` (None: no hole).  Object 1: behind the sheet, its rect the full screen (67 500 pixels, nine
    rounds of 8192): visible only through the hole.  Object 2: behind the sheet beside the hole."""
    W, H = 300, 225
    if hole is None:
        tris = _rect(0, 0, W, H)
    else:
        hx, hy = hole % W, hole // W
        tris = _rect(0, 0, W, hy) + _rect(0, hy + 1, W, H) + _rect(0, hy, hx, hy + 1) + _rect(hx + 1, hy, W, hy + 1)
    sheet = _mesh(W, H, tris, [-0.4 - 0.01 * k for k in range(len(tris))])
    tested = _mesh(W, H, [_box(100, 100, 9, 9)], [-0.9])
    objs = [(sheet, IDENT, *_aabb(W, H, 0, 0, W, H, -0.5, -0.4)),
            (tested, IDENT, *_aabb(W, H, 0, 0, W, H, 0.0, 0.2)),
            (tested, IDENT, *_aabb(W, H, 150, 110, 160, 112, 0.5, 0.6))]
    return _scene(W, H, objs, fv=[2, 1, 0])


@pytest.mark.parametrize("hole", HOLES)
def test_hole_scene_preconditions(oracle_mod, hole):
    s = _hole_scene(hole)
    W, H = s["W"], s["H"]
    _, _, sheet = _oracle().occlusion_pass(W, H, s["view"], s["vp"], s["objs"], [0])
    open_px = np.argwhere(sheet.reshape(-1) == 1.0).reshape(-1).tolist()
    assert open_px == ([] if hole is None else [hole])       # exactly that pixel stays 1.0
    assert sheet[sheet < 1.0].max() < 0.35
    occ, vis, _ = _want(s)
    assert occ.tolist() == ([0, 1, 1] if hole is None else [0, 0, 1])
    assert (W * H + 8191) // 8192 == 9


@pytest.mark.gpu
@pytest.mark.parametrize("hole", HOLES)
def test_hole_scene_exact(oracle_mod, hole):
    _check_gpu(_hole_scene(hole), f"hole {hole}")


# ---- 5. z_near <= depth + eps -------------------------------------------------------------------------
EPS_CASES = [(0.0, False), (1e-4, False), (-1e-3, False), (0.0, True)]


def _z_near_of(z):
    return F(F(z) * F(0.5) + F(0.5))


@functools.lru_cache(maxsize=None)
def _eps_scene(eps, near_plane):
    """64 x 32.  Object 0: a full-screen sheet (on the near plane: stored depth 0).  Objects 1, 2: AABBs
    under it whose z_near is float32(max depth under the rect + eps), visible, and one ulp more, occluded;
    their meshes are degenerate (a valid rect whose triangles are all skipped), so the depth stays the
    sheet's.  On the near plane z_near = 0 comes from a box whose nearer corners (z01 < 0) are dropped;
    no input reaches below 0 (such corners are skipped before the clamp), and the next z_near above 0 is
    2^-25."""
    W, H = 64, 32
    zs = -1.0 if near_plane else 0.3
    sheet = _mesh(W, H, _rect(0, 0, W, H), [[zs, zs, zs]] * 2)
    flat = _mesh(W, H, [[(5, 5), (5, 5), (9, 9)]], [0.0])
    rect = (8, 4, 40, 20)
    base = _scene(W, H, [(sheet, IDENT, *_aabb(W, H, 0, 0, W, H, -3.0, -1.0))], eps=eps)   # key -2: first
    dmax = _want(base)[2][rect[1]:rect[3] + 1, rect[0]:rect[2] + 1].max()
    t_vis = F(dmax + F(eps))
    if near_plane:
        assert dmax == 0.0 and eps == 0.0
        z_vis, z_occ, back = F(-1.0), np.nextafter(F(-1.0), F(0.0)), -1.5
    else:
        t_occ = np.nextafter(t_vis, F(2.0))
        z_vis, z_occ, back = F(2.0) * t_vis - F(1.0), F(2.0) * t_occ - F(1.0), None
        assert _z_near_of(z_vis) == t_vis and _z_near_of(z_occ) == t_occ
    objs = base["objs"] + [(flat, IDENT, *_aabb(W, H, *rect, z, z + 0.125 if back is None else back)) for z in (z_vis, z_occ)]
    s = _scene(W, H, objs, fv=[2, 0, 1], eps=eps)
    s.update(z_near=(_z_near_of(z_vis), _z_near_of(z_occ)), dmax=dmax)
    return s


@pytest.mark.parametrize("eps,near_plane", EPS_CASES)
def test_eps_scene_preconditions(oracle_mod, eps, near_plane):
    s = _eps_scene(eps, near_plane)
    occ, vis, depth = _want(s)
    zv, zo = s["z_near"]
    assert zv == F(s["dmax"] + F(eps)) and zo > zv and (near_plane or zo == np.nextafter(zv, F(2.0)))
    assert occ.tolist() == [0, 0, 1]                         # exactly the two outcomes
    if near_plane:
        assert (depth == 0.0).all() and zv == 0.0 and zo == F(2.0) ** -25


@pytest.mark.gpu
@pytest.mark.parametrize("eps,near_plane", EPS_CASES)
def test_eps_scene_exact(oracle_mod, eps, near_plane):
    _check_gpu(_eps_scene(eps, near_plane), f"eps {eps}")


# ---- 6. visit order -----------------------------------------------------------------------------------
def _cell_objects(n, z_of, aabb_z=(-0.1, 0.1), W=64, H=32):
    """n objects over 8 cells of 16 x 16 pixels; object i's AABB is its cell i % 8 at aabb_z (z_near 0.45
    by default), its mesh fills the cell at z_of(i): an earlier visit of a near mesh hides the cell's later
    objects, so the flags depend on the visit order."""
    objs = []
    for i in range(n):
        cx, cy = 16 * (i % 4), 16 * ((i % 8) // 4)
        mesh = _mesh(W, H, _rect(cx, cy, cx + 16, cy + 16), [z_of(i), z_of(i) + 0.001])
        objs.append((mesh, IDENT, *_aabb(W, H, cx, cy, cx + 15, cy + 15, *aabb_z)))
    return objs


@functools.lru_cache(maxsize=None)
def _order_scene(case):
    W, H = 64, 32
    rng = np.random.default_rng(17)
    near_far = lambda i: -0.5 if i % 3 == 0 else 0.5 - 0.004 * i      # noqa: E731
    if case == "ties40":            # one key for 40 objects (beyond an insertion-sort threshold of 16)
        return _scene(W, H, _cell_objects(40, near_far), fv=rng.permutation(40))
    if case == "signed_zero_keys":  # keys -0.0 and +0.0 compare equal: input order
        view = np.array([1, 0, -0.0, 0, 0, 1, -0.0, 0, 0, 0, 1, 0, 0, 0, -0.0, 1], F)
        objs = _cell_objects(24, near_far)
        objs = [(o[0], o[1], *(o[2:] if i % 2 else (np.r_[o[2][:2], F(-0.0)].astype(F), np.r_[o[3][:2], F(-0.0)].astype(F))))
                for i, o in enumerate(objs)]
        return _scene(W, H, objs, fv=rng.permutation(24), view=view)
    if case == "duplicates_and_out_of_range":
        objs = _cell_objects(12, near_far, aabb_z=(-0.1, 0.1))
        objs = [(o[0], o[1], o[2], o[3] + np.array([0, 0, 0.01 * (i % 5)], F)) for i, o in enumerate(objs)]
        fv = [3, 2 ** 31, 1, 3, 0xFFFFFFFF, 0, 12, 9, 1, 2, 17, 11, 3, 8, 2 ** 31 + 3, 0]
        return _scene(W, H, objs, fv=fv)
    if case == "invalid_rects":     # behind the camera (w = z <= 0.001), off screen, beyond the far plane
        mesh = _mesh(W, H, _rect(0, 0, W, H), [-1.0, -2.0])
        boxes = [((-1, -1, -3), (1, 1, -1)), ((-1, -1, -1), (1, 1, 0.001)), ((3, 0, 1), (4, 1, 2)),
                 ((-9, -9, 1), (-8, -8, 1)), ((0, 5, 2), (1, 6, 3)), ((0, -7, 1), (1, -6, 1))]
        objs = [(mesh, IDENT, np.array(a, F), np.array(b, F)) for a, b in boxes]
        return _scene(W, H, objs, fv=rng.permutation(len(objs)), vp=PERSP)
    if case == "valid_rect_no_triangles":
        flat = _mesh(W, H, [[(5, 5), (5, 5), (9, 9)], [(1, 1), (9, 9), (5, 5)]], [0.0, 0.1])
        objs = _cell_objects(4, near_far) + [(flat, IDENT, *_aabb(W, H, 0, 0, W, H, -0.9, -0.8))]
        return _scene(W, H, objs, fv=[0, 1, 2, 3, 4])
    n = int(case)                   # n = 0 .. 3 objects
    return _scene(W, H, _cell_objects(n, lambda i: 0.3 - 0.25 * i, aabb_z=(0.0, 0.5)), fv=np.arange(n)[::-1])


ORDER_CASES = ["ties40", "signed_zero_keys", "duplicates_and_out_of_range", "invalid_rects", "valid_rect_no_triangles",
               "0", "1", "2", "3"]


@pytest.mark.parametrize("case", ORDER_CASES)
def test_order_scene_preconditions(oracle_mod, case):
    s = _order_scene(case)
    occ, vis, depth = _want(s)
    n, fv = len(s["objs"]), s["fv"]
    key = np.array([(_m4v(s["view"], np.r_[F(0.5) * (o[2] + o[3]), F(1)][None].astype(F)))[0, 2] for o in s["objs"]], F)
    if case in ("ties40", "signed_zero_keys"):
        assert (key == key[0]).all() and not np.array_equal(fv, np.arange(n))
        assert 0 < occ.sum() < n
        # equal keys: the visit order is the input order, and another order gives other flags
        assert vis.tolist() == [i for i in fv.tolist() if not occ[i]]
        occ_r, _, _ = _oracle().occlusion_pass(s["W"], s["H"], s["view"], s["vp"], s["objs"], fv[::-1].copy())
        assert not np.array_equal(occ_r, occ)
        if case == "signed_zero_keys":
            assert set(np.signbit(key).tolist()) == {False, True}
    elif case == "duplicates_and_out_of_range":
        assert (fv >= n).sum() == 5 and len(fv) - len(set(fv.tolist())) >= 4
        seen = vis.tolist()
        assert len(seen) != len(set(seen))                   # visited twice, listed twice
        assert 0 < occ.sum() < n
    elif case == "invalid_rects":
        assert occ.sum() == 0 and sorted(vis.tolist()) == list(range(n)) and (depth == 1.0).all()
    elif case == "valid_rect_no_triangles":
        assert vis[0] == 4 and occ[4] == 0
        alone = _oracle().occlusion_pass(s["W"], s["H"], s["view"], s["vp"], s["objs"], [4])
        assert alone[1].tolist() == [4] and (alone[2] == 1.0).all()
    else:
        assert len(vis) + int(occ.sum()) == n == int(case)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ORDER_CASES)
def test_order_scene_exact(oracle_mod, case):
    _check_gpu(_order_scene(case), case)


@pytest.mark.gpu
def test_empty_frustum_list_and_no_objects(oracle_mod):
    """An empty frustum-visible list over some objects, over none, and a list of out-of-range indices only:
    nothing visited, the depth cleared to 1.0."""
    import shs_gpu
    s3 = _order_scene("3")
    with shs_gpu.Context(0) as ctx:
        for objs, fv in ((s3["objs"], []), ([], []), ([], [0, 7]), (s3["objs"], [3, 99])):
            s = _scene(64, 32, objs, fv=np.asarray(fv, np.uint32))
            got = _gpu(ctx, s)
            _same(got, _want(s), f"{len(objs)} objects, fv {fv}")
            assert len(got[1]) == 0 and (got[2] == 1.0).all()


# ---- 7. one context through a sequence ----------------------------------------------------------------
@pytest.mark.gpu
def test_one_context_through_a_sequence(oracle_mod):
    """Many objects -> one -> none -> many, a large mesh -> a small one, a large buffer -> 1 x 1 -> large,
    a disabled pass in between: every call against the oracle (stale rect, triangle and visible-list
    contents, the two zeroed tail records)."""
    import shs_gpu
    one = _order_scene("1")
    px1 = _scene(1, 1, _order_scene("ties40")["objs"], fv=np.arange(40)[::-1])
    steps = [_order_scene("ties40"), _chunk_scene(2 * 1024 + 37), one, _scene(64, 32, one["objs"], fv=[]),
             _window_scene("c_three_whole_windows"), ("off", _order_scene("duplicates_and_out_of_range")), px1,
             _hole_scene(8192), _chunk_scene(1025), _order_scene("2"), _window_scene("b_straddle_by_one"),
             _order_scene("ties40")]
    with shs_gpu.Context(0) as ctx:
        for k, s in enumerate(steps):
            if isinstance(s, tuple):
                s = s[1]
                got, want = _gpu(ctx, s, enable=False), _want(s, enable=False)
                assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), f"step {k} (disabled)"
                assert got[0].sum() == 0 and got[1].tolist() == [i for i in s["fv"].tolist() if i < len(s["objs"])]
            else:
                _same(_gpu(ctx, s), _want(s), f"step {k}")


# ---- 8. models and meshes -----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _model_scene(case):
    W, H = 256, 128
    rng = np.random.default_rng(23)
    if case == "shared_mesh":       # 30 objects, one 300-triangle mesh (stored in Morton order), own models
        tris = [_box(int(rng.integers(0, 40)), int(rng.integers(0, 30)), int(rng.integers(2, 12)), int(rng.integers(2, 12)))
                for _ in range(300)]
        tris = tris[:298] + _rect(0, 0, 52, 42)              # a backing that covers the AABB's rect
        mesh = _mesh(W, H, tris, np.r_[-0.1 + 0.2 * rng.permutation(298) / 300, 0.1, 0.1])
        objs = []
        for i in range(30):                                 # 15 places: an object deeper in a place is hidden
            dx, dy, dz = 50 * int(rng.integers(0, 5)), 42 * int(rng.integers(0, 3)), float(F(rng.uniform(-0.7, 0.7)))
            m = IDENT.copy()
            m[12:15] = (2.0 * dx / W, 2.0 * dy / H, dz)
            objs.append((mesh, m, *_aabb(W, H, dx, dy, dx + 50, dy + 40, dz - 0.1, dz + 0.1)))
        return _scene(W, H, objs, fv=rng.permutation(30))
    if case == "model_bottom_row":  # the reference takes vec3(model * v): the model's w row is dropped
        mesh = _mesh(W, H, _rect(20, 10, 120, 90) + [_box(150, 20, 40, 50)], [0.1, 0.11, -0.3])
        m = IDENT.copy()
        m[3], m[7], m[11], m[15] = 0.25, -0.5, 0.125, 3.0
        m[12:15] = (2.0 * 8 / W, 2.0 * 4 / H, 0.05)
        back = _mesh(W, H, [_box(1, 1, 3, 3)], [0.9])
        objs = [(mesh, m, *_aabb(W, H, 28, 14, 128, 94, 0.1, 0.2)),
                (back, IDENT, *_aabb(W, H, 40, 30, 100, 80, 0.6, 0.7)),
                (back, IDENT, *_aabb(W, H, 0, 0, 100, 80, 0.7, 0.8))]
        return _scene(W, H, objs, fv=[2, 1, 0])
    # an index >= n_verts: shs_mesh_upload takes the mesh, the pass skips that triangle
    tris = _rect(10, 10, 60, 60) + [_box(100, 30, 30, 30), _box(150, 60, 20, 20)]
    idx = np.arange(12, dtype=np.uint32)
    idx[7] = 12                      # triangle 2: one past the last vertex
    idx[9] = 0xFFFFFFFF              # triangle 3
    mesh = _mesh(W, H, tris, [0.1, 0.12, -0.4, -0.5], idx=idx)
    return _scene(W, H, [(mesh, IDENT, *_aabb(W, H, 0, 0, W, H, -0.5, 0.1))])


MODEL_CASES = ["shared_mesh", "model_bottom_row", "index_out_of_range"]


@pytest.mark.parametrize("case", MODEL_CASES)
def test_model_scene_preconditions(oracle_mod, case):
    s = _model_scene(case)
    occ, vis, depth = _want(s)
    if case == "shared_mesh":
        assert len({id(o[0]) for o in s["objs"]}) == 1 and 0 < occ.sum() < 30
    elif case == "model_bottom_row":
        assert occ.tolist() == [0, 1, 0]
        # the mesh lands where the model's upper three rows put it: 8 pixels right, 4 up
        assert depth[14:94, 28:128].max() < 1.0 and depth[50, 20] == 1.0
        cnt, _ = _tri_counts(s["objs"][0][0], s["objs"][0][1], IDENT, s["W"], s["H"])
        assert cnt.tolist() == [101 * 81, 101 * 81, 40 * 50]
    else:
        mesh = s["objs"][0][0]
        cnt, reason = _tri_counts(mesh, IDENT, IDENT, s["W"], s["H"])
        assert reason.tolist() == [LIVE, LIVE, SKIP_INDEX, SKIP_INDEX]
        assert (depth[30:60, 100:130] == 1.0).all() and (depth < 1.0).sum() == 50 * 50


@pytest.mark.gpu
@pytest.mark.parametrize("case", MODEL_CASES)
def test_model_scene_exact(oracle_mod, case):
    _check_gpu(_model_scene(case), case)


# ---- 9. buffers over 2^31 pixels ----------------------------------------------------------------------
@pytest.mark.gpu
def test_buffer_over_2_31_pixels_is_rejected(oracle_mod):
    """k_occlusion indexes a triangle's pairs and a rect's pixels with 32-bit ints, so the ABI rejects
    width * height > 2^31 (in fact from 2^31 - 2^16 on: the strided loops overshoot) with an error string,
    before anything is allocated (a 65535 x 65535 float buffer would be 17 GB)."""
    import ctypes

    import shs_gpu
    from shs_gpu import _abi
    s = _order_scene("2")
    assert 46341 * 46341 > 2 ** 31 and 65535 * 32769 > 2 ** 31

    def call(ctx, W, H):   # the C entry point with depth = NULL: the host allocates nothing W * H either
        d = _abi.OcclusionDescC()
        d.width, d.height, d.depth_epsilon, d.enable = W, H, 1e-4, 1
        for k in range(16):
            d.view[k], d.view_proj[k] = float(IDENT[k]), float(IDENT[k])
        objs = (_abi.OccluderC * 1)()
        objs[0].mesh_id = ctx.upload_lib_mesh(s["objs"][0][0])
        fv, occ, vis, nv = (ctypes.c_uint32 * 1)(0), (ctypes.c_uint8 * 1)(), (ctypes.c_uint32 * 1)(), ctypes.c_int32()
        ctx._check(ctx._lib.shs_occlusion_pass(ctx._h, ctypes.byref(d), objs, 1, ctypes.cast(fv, ctypes.c_void_p), 1,
                                               ctypes.cast(occ, ctypes.c_void_p), ctypes.cast(vis, ctypes.c_void_p),
                                               ctypes.byref(nv), None))
        return nv.value

    with shs_gpu.Context(0) as ctx:
        for W, H in ((65535, 65535), (65535, 32769), (32769, 65535), (46341, 46341), (65534, 32769)):
            with pytest.raises(shs_gpu.ShsError, match="2\\^31"):
                call(ctx, W, H)
        assert call(ctx, 64, 32) == 1
        _same(_gpu(ctx, s), _want(s), "after the rejections")   # the context is still good
