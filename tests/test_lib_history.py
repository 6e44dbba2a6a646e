"""Library passes under a known, inconsistent history.

A camera or shadow pass chooses how it rasters from what an earlier pass of the same context measured
(shs_lib_plan.hpp plan_lib_pass, shs_abi_lib.cpp check_pass), not from the pass in front of it:

  * shallow raster (256-candidate rounds) when the last checked pass's fullest bin list was <= 256 (scan
    mode: its primitive count), else the deep one (1024); a context's first pass runs deep;
  * k_lib_dyn / k_lib_hsort sort a bin list only when that pass had a list over 1024 entries (or none was
    checked yet), the pass is deep and unsplit, and 1024 < n <= min(bin_cap, 8192);
  * bin_cap starts at 256 and grows to next_pow2(last max); the spill list starts at 65,536 entries; the
    clipped-extra capacity is sized by the first pass (max(4096, triangles / 4));
  * the statistics refresh only at a finish, and the shadow pass keeps its own copy of all of it.

Every context here is fresh, so each pass's variant is known from the sequence alone; every rendered
frame must equal the oracle's (depth bit-exact, HDR / motion within 1e-5, the triangle counts and the
covered pixels equal), whatever the earlier passes predicted.

Scenes (256x192, identity viewproj, NDC-space soups): a *stack* is N small triangles whose corners lie
within 9 px of a bin tile's centre, so that tile's list is exactly the stack; 600 padding triangles far
from it put the pass into bin mode; a *lid* (two triangles on the nearest depth plane, a later draw)
fills the whole tile at the front of a sorted list, so the sorted raster's early exit runs while stack
triangles on the same plane, submitted earlier, still win their pixels by the tie rule.  Large primitives
are binned after the small ones, so the lid ends an unsorted list; the *floor* variants add the tile's own
square on the middle plane before the stack: an unsorted list then covers the tile near its start, and a
raster that took it for a sorted one (a stale hsr range, k_lib_dyn's predicate and the raster's apart)
ends its rounds early and drops the winners behind -- checked by breaking k_lib_dyn's predicate once:
test_bin_cap_edges[True] then fails on the 2049-entry list after the 2048-entry one."""
import numpy as np
import pytest

from helpers import assert_depth_bitexact, assert_float_close

W, H, T = 256, 192, 32
CX, CY = 112, 80                     # the stack's centre: the middle of bin tile (3, 2)
CLEAR = (0.1, 0.2, 0.3, 1.0)
N_PAD = 600
N_S, N_L, N_M, N_H = 200, 150, 3000, 9000   # stack sizes of the named scenes


# ---- scenes -------------------------------------------------------------------------------------
class Scene:
    def __init__(self, name, frame, draws, n_list=None):
        self.name, self.frame, self.draws = name, frame, draws
        self.n_list = n_list          # the fullest bin list (the stack tile's), where it is exact


def _tris(rng, cx, cy, spread, n, w, h, zlo=-0.5):
    """n triangles (circumradius 2-3 px, so every one covers pixel centres) whose centres lie within
    `spread` px of (cx, cy) per axis; three exact depth planes, 30 % scattered behind the nearest."""
    c = np.stack([cx + rng.uniform(-spread[0], spread[0], n), cy + rng.uniform(-spread[1], spread[1], n)], axis=1)
    r = rng.uniform(2.0, 3.0, n)
    a = rng.uniform(0.0, 2.0 * np.pi, n)[:, None] + np.arange(3)[None, :] * (2.0 * np.pi / 3.0)
    px = c[:, None, :] + r[:, None, None] * np.stack([np.cos(a), np.sin(a)], axis=2)
    z = np.float32([zlo, 0.0, 0.5])[rng.integers(0, 3, n)]
    z = np.where(rng.random(n) < 0.3, rng.uniform(zlo, 0.9, n).astype(np.float32), z)
    pos = np.empty((n, 3, 3), np.float32)
    pos[..., 0] = px[..., 0] * (2.0 / w) - 1.0
    pos[..., 1] = px[..., 1] * (2.0 / h) - 1.0
    pos[..., 2] = z[:, None]
    pos = pos.reshape(-1, 3)
    return pos, rng.normal(size=pos.shape).astype(np.float32)   # distinct normals: the winner shows


def _stack(rng, n, cx=CX, cy=CY, w=W, h=H):
    return _tris(rng, cx, cy, (6.0, 6.0), n, w, h)


def _padding(rng, n, w=W, h=H):
    """Far from every stack: x NDC in 0.5 .. 0.9."""
    return _tris(rng, 0.85 * w, 0.5 * h, (0.1 * w - 3.0, 0.45 * h), n, w, h)


def _lid_mesh(cx=CX, cy=CY, w=W, h=H, y0=None, y1=None, z=-0.5, half=24.0):
    from shs_gpu.lib_path import LibMesh
    x0, x1 = cx - half, cx + half
    y0, y1 = (cy - half if y0 is None else y0), (cy + half if y1 is None else y1)
    q = np.float32([[x0, y0], [x1, y0], [x1, y1], [x0, y0], [x1, y1], [x0, y1]])
    pos = np.empty((6, 3), np.float32)
    pos[:, 0] = q[:, 0] * (2.0 / w) - 1.0
    pos[:, 1] = q[:, 1] * (2.0 / h) - 1.0
    pos[:, 2] = z
    return LibMesh(pos, np.tile(np.float32([0.3, 0.5, -0.8]), (6, 1)))


def _frame(w=W, h=H):
    from shs_gpu.lib_path import LibFrame
    return LibFrame(w, h, depth_motion=True, zn=1.0, zf=1.0, bg_gradient=False, clear_hdr=CLEAR)


def _stack_scene(name, n_stack, n_pad=N_PAD, lid=True, seed=None, w=W, h=H, cx=CX, cy=CY, lid_y=(None, None), floor=False):
    from shs_gpu.lib_path import LibDraw, LibMesh
    rng = np.random.default_rng(1000 + n_stack if seed is None else seed)
    draws = []
    if n_pad:
        draws.append(LibDraw(mesh=LibMesh(*_padding(rng, n_pad, w, h)), program=2, cull_mode=0))
    if floor:
        # The bin tile's own square (every pixel centre of it, small enough to be binned with the stack's
        # triangles, not with the large primitives after them) on the middle plane, submitted before the
        # stack: the unsorted list covers the tile near its start with something half of the list lies
        # behind and a third in front of -- a raster that took that list for a sorted one would end its
        # rounds on an entry behind it and drop the winners further on.
        # (screen x = (ndc + 1) / 2 * (w - 1), pixel centres at + 0.5: the square in screen units)
        fcx, fcy = (cx // T * T + T / 2) * w / (w - 1), (cy // T * T + T / 2) * h / (h - 1)
        draws.append(LibDraw(mesh=_lid_mesh(fcx, fcy, w, h, z=0.0, half=T / 2 - 0.2), program=2, cull_mode=0,
                             base_color=(0.2, 0.8, 0.4)))
    draws.append(LibDraw(mesh=LibMesh(*_stack(rng, n_stack, cx, cy, w, h)), program=2, cull_mode=0))
    if lid:
        draws.append(LibDraw(mesh=_lid_mesh(cx, cy, w, h, *lid_y), program=3, cull_mode=0, base_color=(0.9, 0.3, 0.2)))
    return Scene(name, _frame(w, h), draws, n_stack + (2 if lid else 0) + (2 if floor else 0))


def _list_scene(n_list, floor=False):
    """Stack + lid (+ floor) whose tile list is exactly n_list entries."""
    return _scene(f"len{n_list}{'f' if floor else ''}", lambda name: _stack_scene(name, n_list - (4 if floor else 2), floor=floor))


def _clip_soup(rng, n):
    """Random world-space triangles around a perspective camera (test_lib_parity._clip_soup): many cross
    the near / far / side planes, some lie behind the eye, some are degenerate."""
    c = rng.uniform([-12, -8, -2], [12, 8, 40], size=(n, 1, 3))
    tris = c + rng.normal(scale=rng.choice([0.3, 2.0, 9.0], size=(n, 1, 1)), size=(n, 3, 3))
    tris[: n // 20, 2] = tris[: n // 20, 0] + 1e-4 * rng.normal(size=(n // 20, 3))
    pos = tris.reshape(-1, 3).astype(np.float32)
    return pos, rng.normal(size=pos.shape).astype(np.float32), rng.uniform(-2, 2, size=(pos.shape[0], 2)).astype(np.float32)


def _clip_draw(n, seed):
    from shs_gpu.lib_path import LibDraw, LibMesh, look_at_lh, mat_mul, perspective_lh_no
    view = look_at_lh((0.3, 0.7, -3.0), (0.0, 0.0, 10.0))
    proj = perspective_lh_no(np.float32(np.deg2rad(60.0)), np.float32(W) / np.float32(H), 0.5, 30.0)
    pos, nrm, uv = _clip_soup(np.random.default_rng(seed), n)
    return LibDraw(mesh=LibMesh(pos, nrm, uv), program=1, viewproj=mat_mul(proj, view), camera_pos=(0.3, 0.7, -3.0),
                   cull_mode=0, light_intensity=3.0)


N_C, N_C_BIG = 1200, 20000


def _build(name):
    if name == "S":   # scan mode: at most 512 triangles in all
        return _stack_scene("S", N_S, n_pad=300)
    if name == "L":
        return _stack_scene("L", N_L)
    if name in ("M", "Mf"):
        return _stack_scene(name, N_M, floor=name == "Mf")
    if name in ("H", "Hf"):
        return _stack_scene(name, N_H, floor=name == "Hf")
    if name == "E":
        return Scene("E", _frame(), [])
    if name == "C":
        return Scene("C", _frame(), [_clip_draw(N_C, 21)])
    if name == "CM":  # the clip soup, enough of it to overflow the first pass's clipped-extra capacity, and a stack
        m = _stack_scene("CM", N_M)
        return Scene("CM", _frame(), [_clip_draw(N_C_BIG, 22)] + m.draws)
    if name == "TEN":
        return _ten_stacks()
    if name in ("M96", "M96f"):  # the stack scene for a 96x64 frame: bin tile (1, 0); the lid ends on the frame's edge
        return _stack_scene(name, N_M, w=96, h=64, cx=48, cy=16, lid_y=(0, 40), floor=name == "M96f")
    raise KeyError(name)


TEN_N = 8000
TEN_CENTRES = [(T * tx + T // 2, T * ty + T // 2) for ty in (1, 4) for tx in range(5)]


def _ten_stacks():
    from shs_gpu.lib_path import LibDraw, LibMesh
    rng = np.random.default_rng(77)
    parts = [_stack(rng, TEN_N, cx, cy) for cx, cy in TEN_CENTRES]
    pos = np.concatenate([p for p, _ in parts])
    nrm = np.concatenate([n for _, n in parts])
    draws = [LibDraw(mesh=LibMesh(*_padding(rng, N_PAD)), program=2, cull_mode=0),
             LibDraw(mesh=LibMesh(pos, nrm), program=2, cull_mode=0)]
    return Scene("TEN", _frame(), draws, TEN_N)


_SCENES, _REFS = {}, {}


def _scene(name, make=_build):
    if name not in _SCENES:
        _SCENES[name] = make(name)
    return _SCENES[name]


def _pick(name, floor):
    """The named scene, or its variant with a floor under the stack (M, H and the 96x64 M)."""
    return _scene(name + "f" if floor and name in ("M", "H", "M96") else name)


def _ref(oracle_mod, sc):
    """The oracle's result of a scene, rendered once per module and never written to."""
    if sc.name not in _REFS:
        rh, rd, rm, rst = oracle_mod.pbr_forward(sc.frame, sc.draws, None)
        for a in (rh, rd, rm):
            a.setflags(write=False)
        rst["covered_pixels"] = int((rd < 1.0).sum())
        _REFS[sc.name] = (rh, rd, rm, rst)
    return _REFS[sc.name]


# ---- the host's rule, restated (the expected variant of a pass from the last checked one) -----------
class HostRule:
    """What plan_lib_pass decides from the statistics check_pass left (camera pass)."""

    def __init__(self):
        self.checked, self.maxbin, self.extra, self.bin_cap, self.part = False, 0, 0, 256, 0

    def predict(self, sc):
        n_tris = sum(d.mesh.n_tris for d in sc.draws)
        scan = n_tris <= 512
        fullest = n_tris + self.extra if scan else self.maxbin
        shallow = self.checked and fullest <= 256
        part = 0 if scan else self.part
        hsort = (not scan) and not part and not shallow and (not self.checked or self.maxbin > 1024)
        return dict(scan=scan, shallow=shallow, hsort=hsort, part=part, bin_cap=self.bin_cap)

    def checked_pass(self, st):
        self.checked, self.maxbin, self.extra = True, st["max_tile_bin"], st["clipped_extra"]
        if self.maxbin > self.bin_cap:
            self.bin_cap = 1 << (self.maxbin - 1).bit_length()


def _expected_rounds(v, n):
    """(candidate rounds over a list of n entries -- the only one past bin_cap, so a spilling tile's items
    are its own n -- when no early exit ends it; whether the raster takes the list for sorted)."""
    cand = 256 if v["shallow"] else 1024
    gsorted = (not v["shallow"]) and v["hsort"] and not v["part"] and 1024 < n <= min(v["bin_cap"], 8192)
    return -(-n // cand), gsorted


# ---- rendering and checking ---------------------------------------------------------------------
def _check(ctx, oracle_mod, sc, render=True):
    if render:
        ctx.render_pbr_forward(sc.frame, sc.draws)
    gh, gd, gm = ctx.resolve_lib()
    st = ctx.lib_stats()
    rh, rd, rm, rst = _ref(oracle_mod, sc)
    assert_depth_bitexact(gd, rd)
    assert_float_close(gm, rm, what=f"{sc.name} motion")
    assert_float_close(gh, rh, what=f"{sc.name} hdr")
    for k in ("tri_input", "tri_after_clip", "tri_raster", "covered_pixels"):
        assert st[k] == rst[k], (sc.name, k, st[k], rst[k])
    if sc.n_list is not None and st["tri_input"] > 512:
        assert st["max_tile_bin"] == sc.n_list, (sc.name, st["max_tile_bin"], sc.n_list)
    return st


@pytest.fixture
def ctx():
    import shs_gpu
    c = shs_gpu.Context(0)
    try:
        yield c
    finally:
        c.close()


def _all_pairs_walk(names):
    """A closed walk over the complete directed graph with loops on `names` (Hierholzer): every ordered
    pair of scenes, self-pairs included, exactly once as consecutive frames."""
    out = {a: list(reversed(names)) for a in names}
    stack, walk = [names[0]], []
    while stack:
        v = stack[-1]
        if out[v]:
            stack.append(out[v].pop())
        else:
            walk.append(stack.pop())
    return walk[::-1]


# ---- scene conditions (no GPU) --------------------------------------------------------------------
def _named(name):
    return _list_scene(int(name[3:].rstrip("f")), name.endswith("f")) if name.startswith("len") else _scene(name)


def _tile_of(cx, cy):
    return (cx // T) * T, (cy // T) * T


def _covered_box(depth):
    ys, xs = np.nonzero(depth < 1.0)
    return xs.min(), xs.max(), ys.min(), ys.max()


@pytest.mark.parametrize("name", ["S", "L", "M", "H", "M96", "len256", "len257", "len1024", "len1025", "len2048",
                                  "len2049", "len8192", "len8193", "len1025f", "len2049f", "len8192f", "Mf", "Hf", "M96f"])
def test_stack_lies_inside_its_bin_tile(oracle_mod, name):
    """The stack's corners, and the pixels the oracle covers with it, lie in the interior of one bin tile
    (so that tile's list is the stack and nothing else), and the padding is nowhere near it."""
    sc = _named(name)
    w, h = sc.frame.width, sc.frame.height
    stack = sc.draws[-2]
    cx, cy = (48, 16) if name.startswith("M96") else (CX, CY)
    tx0, ty0 = _tile_of(cx, cy)
    p = stack.mesh.positions
    px, py = (p[:, 0] + 1.0) * 0.5 * w, (p[:, 1] + 1.0) * 0.5 * h
    assert px.min() >= cx - 9 and px.max() <= cx + 9 and py.min() >= cy - 9 and py.max() <= cy + 9
    assert tx0 + 2 <= px.min() and px.max() <= tx0 + T - 2 and ty0 + 2 <= py.min() and py.max() <= ty0 + T - 2
    _, rd, _, rst = oracle_mod.pbr_forward(sc.frame, [stack], None)
    assert rst["tri_raster"] == stack.mesh.n_tris          # every stack triangle reaches the raster
    x0, x1, y0, y1 = _covered_box(rd)
    assert tx0 < x0 and x1 < tx0 + T - 1 and ty0 < y0 and y1 < ty0 + T - 1, (x0, x1, y0, y1)   # (rows y-up, as NDC)
    pad = sc.draws[0].mesh.positions
    assert ((pad[:, 0] + 1.0) * 0.5 * w).min() >= tx0 + T + 4   # in other columns of bin tiles


def test_ten_stacks_each_inside_its_own_tile():
    sc = _scene("TEN")
    p = sc.draws[1].mesh.positions.reshape(len(TEN_CENTRES), -1, 3)
    assert p.shape[1] == 3 * TEN_N
    tiles = set()
    for (cx, cy), q in zip(TEN_CENTRES, p):
        tx0, ty0 = _tile_of(cx, cy)
        px, py = (q[:, 0] + 1.0) * 0.5 * W, (q[:, 1] + 1.0) * 0.5 * H
        assert tx0 + 2 <= px.min() and px.max() <= tx0 + T - 2 and ty0 + 2 <= py.min() and py.max() <= ty0 + T - 2
        tiles.add((tx0, ty0))
    assert len(tiles) == len(TEN_CENTRES) == 10
    pad = sc.draws[0].mesh.positions
    assert ((pad[:, 0] + 1.0) * 0.5 * W).min() > max(cx for cx, _ in TEN_CENTRES) + T
    # the first attempt's spill: every list's entries past the initial bin capacity
    assert len(TEN_CENTRES) * (TEN_N - 256) > 65536


@pytest.mark.parametrize("name", ["M", "H", "len1025", "len8192", "M96", "len1025f", "len2049f", "len8192f", "Mf", "Hf", "M96f"])
def test_lid_fills_the_tile_and_stack_triangles_win_ties(oracle_mod, name):
    sc = _named(name)
    rh, rd, _, _ = _ref(oracle_mod, sc)
    lh, ld, _, _ = oracle_mod.pbr_forward(sc.frame, [sc.draws[-1]], None)
    tile = ld == np.float32(0.25)
    h = sc.frame.height
    cx, cy = (48, 16) if name.startswith("M96") else (CX, CY)
    tx0, ty0 = _tile_of(cx, cy)
    box = np.zeros_like(tile)
    box[ty0:ty0 + T, tx0:tx0 + T] = True
    assert tile[box].all() and box.sum() == T * T            # the lid covers the whole bin tile
    assert (rd[box] == np.float32(0.25)).all()                # nothing lies in front of it
    won = (rh[box] != lh[box]).any(axis=-1)
    assert won.sum() >= 200, int(won.sum())                   # stack triangles of the lid's plane win their pixels


@pytest.mark.parametrize("name", ["len1025f", "len2049f", "len8192f", "Mf", "Hf", "M96f"])
def test_floor_covers_its_tile_and_no_other_column(oracle_mod, name):
    sc = _named(name)
    W, H = sc.frame.width, sc.frame.height
    floor = sc.draws[1]
    assert floor.mesh.n_tris == 2 and sc.draws[2].mesh.n_tris == sc.n_list - 4
    _, fd, _, _ = oracle_mod.pbr_forward(sc.frame, [floor], None)
    tx0, ty0 = _tile_of(*((48, 16) if name == "M96f" else (CX, CY)))
    box = np.zeros(fd.shape, bool)
    box[ty0:ty0 + T, tx0:tx0 + T] = True
    assert np.array_equal(fd == np.float32(0.5), box)       # the tile's pixels and no others
    sx = (floor.mesh.positions[:, 0] + 1.0) * 0.5 * (W - 1)
    sy = (floor.mesh.positions[:, 1] + 1.0) * 0.5 * (H - 1)
    for lo, hi, t0 in ((sx.min(), sx.max(), tx0), (sy.min(), sy.max(), ty0)):
        assert t0 <= lo and hi <= t0 + T                     # its box: the tile and at most the next one


def test_clip_soup_crosses_the_near_plane():
    for name in ("C", "CM"):
        d = _scene(name).draws[0]
        m = np.asarray(d.viewproj, np.float64).reshape(4, 4).T      # column-major
        p = np.concatenate([d.mesh.positions.astype(np.float64), np.ones((d.mesh.positions.shape[0], 1))], axis=1)
        c = (p @ m.T).reshape(-1, 3, 4)
        inside = c[..., 2] >= -c[..., 3]
        crossing = inside.any(axis=1) & ~inside.all(axis=1)
        assert crossing.sum() > 20, int(crossing.sum())


def test_walk_holds_every_ordered_pair():
    names = ["L", "S", "M", "H", "E", "C"]
    walk = _all_pairs_walk(names)
    assert len(walk) == 37 and walk[0] == walk[-1] == "L"
    assert set(zip(walk, walk[1:])) == {(a, b) for a in names for b in names}


# ---- 1: every transition --------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("floor", [False, True])
def test_every_transition(ctx, oracle_mod, floor):
    names = ["L", "S", "M", "H", "E", "C"]
    walk = _all_pairs_walk(names)
    assert set(zip(walk, walk[1:])) == {(a, b) for a in names for b in names}
    seen = []
    for name in walk:
        sc = _pick(name, floor)
        st = _check(ctx, oracle_mod, sc)
        seen.append((name, st["max_tile_bin"], st["spilled"], st["clipped_extra"]))
        if name == "L":
            assert st["max_tile_bin"] <= 256
        if name in ("M", "H"):
            assert st["max_tile_bin"] == sc.n_list == {"M": N_M, "H": N_H}[name] + (4 if floor else 2)
        if name == "C":
            assert st["clipped_extra"] > 0
    print("walk:", seen)


# ---- 2: stale statistics ----------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("floor", [False, True])
@pytest.mark.parametrize("first,rest", [("L", "H"), ("L", "HM"), ("L", "HML"), ("L", "HMLM"),
                                        ("H", "L"), ("H", "LS"), ("H", "LSM")])
def test_stale_statistics(ctx, oracle_mod, first, rest, floor):
    """Frames enqueued back to back choose their variant from the last finished frame's statistics; the
    last one is resolved and checked."""
    _check(ctx, oracle_mod, _pick(first, floor))
    for name in rest:
        sc = _pick(name, floor)
        ctx.render_pbr_forward(sc.frame, sc.draws)
    _check(ctx, oracle_mod, _pick(rest[-1], floor), render=False)


# ---- 3: exact list lengths --------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("floor", [False, True])
@pytest.mark.parametrize("n", [256, 257, 1024, 1025, 8192, 8193])
def test_exact_list_lengths(ctx, oracle_mod, n, floor):
    """Pass 1: bin_cap 256 (the longer lists spill); pass 2: the grown bin_cap, sorted where eligible;
    pass 3: steady state."""
    sc = _list_scene(n, floor)
    spilled = []
    for _ in range(3):
        st = _check(ctx, oracle_mod, sc)
        assert st["max_tile_bin"] == n
        spilled.append(st["spilled"])
    assert spilled == [max(n - 256, 0), 0, 0], spilled
    print("exact", n, "spilled", spilled)


# ---- 4: bin_cap edges ---------------------------------------------------------------------------------
BIN_CAP_EDGE_LENGTHS = [1024, 1024, 1025, 1025, 2048, 2049, 2049]
BIN_CAP_EDGE_SPILL = [1024 - 256, 0, 1, 0, 0, 1, 0]   # bin_cap 256, 1024, 1024, 2048, 2048, 2048, 4096


@pytest.mark.gpu
@pytest.mark.parametrize("floor", [False, True])
def test_bin_cap_edges(ctx, oracle_mod, floor):
    spilled = []
    for n in BIN_CAP_EDGE_LENGTHS:
        st = _check(ctx, oracle_mod, _list_scene(n, floor))
        spilled.append(st["spilled"])
    assert spilled == BIN_CAP_EDGE_SPILL, spilled


# ---- 5: spill re-issue -----------------------------------------------------------------------------
@pytest.mark.gpu
def test_spill_overflow_reissue(ctx, oracle_mod):
    ctx.enable_timing(True)     # counts the enqueued passes: a re-issue shows as a second camera pass
    ctx.lib_timing_reset()
    st = _check(ctx, oracle_mod, _scene("TEN"))
    n_pass, _ = ctx.lib_timing_read()
    assert n_pass["camera"] == 2, n_pass      # 77,440 spilled entries > 65,536: re-issued once
    assert st["max_tile_bin"] == TEN_N and st["spilled"] == 0   # the re-issue's bin_cap holds every list
    _check(ctx, oracle_mod, _scene("L"))
    _check(ctx, oracle_mod, _scene("M"))
    n_pass, _ = ctx.lib_timing_read()
    assert n_pass["camera"] == 4, n_pass


# ---- 6: the variant changes across a re-issue ------------------------------------------------------
@pytest.mark.gpu
def test_variant_changes_across_reissue(ctx, oracle_mod):
    """L (statistics: shallow, no sorting), then the clip soup + stack: its first attempt runs shallow and
    overflows the clipped-extra capacity the first pass sized (4096), its re-issue runs deep with sorting
    from the failed attempt's statistics; then L again."""
    ctx.enable_timing(True)
    ctx.lib_timing_reset()
    _check(ctx, oracle_mod, _scene("L"))
    st = _check(ctx, oracle_mod, _scene("CM"))
    assert st["clipped_extra"] > 4096, st
    assert st["max_tile_bin"] > 1024
    n_pass, _ = ctx.lib_timing_read()
    assert n_pass["camera"] == 3, n_pass
    _check(ctx, oracle_mod, _scene("L"))
    print("reissue: clipped_extra", st["clipped_extra"], "max_tile_bin", st["max_tile_bin"])


# ---- 7: part splitting toggled -----------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("floor", [False, True])
def test_part_splitting_toggled(ctx, oracle_mod, floor):
    for part, name in [(0, "M"), (64, "M"), (0, "M"), (0, "H"), (0, "L")]:
        ctx.set_lib_part(part)
        _check(ctx, oracle_mod, _pick(name, floor))


# ---- 8: grid change under history --------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("floor", [False, True])
def test_grid_change_under_history(ctx, oracle_mod, floor):
    for name in ["M", "M96", "M", "E", "M"]:
        _check(ctx, oracle_mod, _pick(name, floor))


# ---- 9: the shadow pass's own history ----------------------------------------------------------------
SHADOW_SIZE = 128
_SHADOW_SETS = {}


def _shadow_set(oracle_mod, name):
    """C5's camera frame at 256x144 over one of four caster sets: `small` (the floor: 512 primitives, scan
    mode), `medium` (+ Suzanne: the fullest list between 256 and 1024), `dense` / `denser` (+ a cluster of
    1,500 / 6,000 triangles of ~3 world units over a few shadow-map texels: lists over 1024).  The oracle's
    shadow map and camera frame, rendered once."""
    if name not in _SHADOW_SETS:
        from shs_gpu import scene_lib
        from shs_gpu.lib_path import IDENTITY, LibMesh, ShadowCaster
        frame, draws, casters, sun, _ = scene_lib.c5_scene(256, 144, SHADOW_SIZE)
        if name == "small":
            casters = casters[:1]
        elif name != "medium":
            n = {"dense": 1500, "denser": 6000}[name]
            rng = np.random.default_rng(n)
            c = rng.uniform([-3.0, 3.0, -3.0], [3.0, 6.0, 3.0], size=(n, 1, 3))
            pos = (c + rng.normal(scale=1.5, size=(n, 3, 3))).reshape(-1, 3).astype(np.float32)
            casters = casters + [ShadowCaster(LibMesh(pos), IDENTITY.copy())]
        sm, lvp = oracle_mod.shadow_map(SHADOW_SIZE, sun, casters)
        scene_lib.wire_shadow(draws, lvp)
        rh, rd, rm, rst = oracle_mod.pbr_forward(frame, draws, sm)
        rst["covered_pixels"] = int((rd < 1.0).sum())
        for a in (sm, lvp, rh, rd, rm):
            a.setflags(write=False)
        _SHADOW_SETS[name] = (frame, draws, casters, sun, sm, lvp, (rh, rd, rm, rst))
    return _SHADOW_SETS[name]


@pytest.mark.gpu
def test_shadow_pass_history(ctx, oracle_mod):
    ctx.set_timeline(True, shadow=True)
    F = {k: i for i, k in enumerate(ctx.LIB_TIMELINE_FIELDS)}
    seen, last = [], {}
    for name in ["small", "denser", "small", "medium", "dense", "denser", "medium", "small"]:
        frame, draws, casters, sun, sm_ref, lvp_ref, (rh, rd, rm, rst) = _shadow_set(oracle_mod, name)
        lvp = ctx.render_shadow_map(SHADOW_SIZE, sun, casters)
        assert np.array_equal(lvp.view(np.uint32), lvp_ref.view(np.uint32)), "light camera differs"
        assert_depth_bitexact(ctx.resolve_shadow_map(), sm_ref)
        t = ctx.lib_debug_timeline().astype(np.int64)
        fullest = int(t[:, F["mt_items"]].max())      # (a lower bound: each workgroup's longest tile)
        seen.append((name, fullest, int(t[:, F["mt_rounds"]].max())))
        last[name] = fullest
        n_tris = sum(c.mesh.n_tris for c in casters)
        if name == "small":
            assert n_tris <= 512 and fullest == n_tris   # scan mode: every primitive is a candidate
        else:
            assert n_tris > 512
        ctx.render_pbr_forward(frame, draws)
        gh, gd, gm = ctx.resolve_lib()
        st = ctx.lib_stats()
        assert_depth_bitexact(gd, rd)
        assert_float_close(gm, rm, what=f"{name} motion")
        assert_float_close(gh, rh, what=f"{name} hdr")
        for k in ("tri_input", "tri_after_clip", "tri_raster", "covered_pixels"):
            assert st[k] == rst[k], (name, k, st[k], rst[k])
    # the sets' densities, from each one's last visit (the bin capacity has grown by then, so the tile's
    # items are its own list and no spilled entries of other tiles)
    assert 256 < last["medium"] <= 1024 < last["dense"] and last["denser"] > 1024, last
    print("shadow (set, longest list seen, rounds):", seen)


# ---- 10: the paths are live --------------------------------------------------------------------------
def _stack_tile_slots(ctx, n_items):
    """(mt_rounds, mt_breaks) of the workgroups whose longest tile was a raster tile of the stack's bin
    tile (its list: n_items entries)."""
    t = ctx.lib_debug_timeline().astype(np.int64)
    F = {k: i for i, k in enumerate(ctx.LIB_TIMELINE_FIELDS)}
    rows = t[t[:, F["mt_items"]] == n_items]
    assert len(rows) >= 1, (n_items, sorted(set(t[:, F["mt_items"]].tolist()))[-5:])
    return rows[:, F["mt_rounds"]], rows[:, F["mt_breaks"]]


def _timeline_pass(ctx, oracle_mod, rule, sc, log):
    """One checked frame under the timeline; -> (the variant the host rule predicts, rounds, sorted)."""
    v = rule.predict(sc)
    st = _check(ctx, oracle_mod, sc)
    rule.checked_pass(st)
    n = sc.n_list
    rounds, breaks = _stack_tile_slots(ctx, n)
    full, gsorted = _expected_rounds(v, n)
    log.append((sc.name, "shallow" if v["shallow"] else "deep", "sorted" if gsorted else "unsorted",
                f"bin_cap={v['bin_cap']}", f"spilled={st['spilled']}", f"rounds={sorted(set(rounds.tolist()))}/{full}",
                f"breaks<={int(breaks.max())}"))
    if gsorted:
        # The early exit reads the waves' key maxima of the tile's last staging pass, stale upwards by
        # design: a raster tile whose first round is one staging pass (the bin tile's outer rows, the lid
        # and a few stack triangles) may run every round; the rows through the stack (several passes in
        # the first round) end before the list does.
        assert (rounds <= full).all() and (rounds * 1024 < n).any(), (sc.name, rounds, n)
    else:
        assert (rounds == full).all(), (sc.name, rounds, full)
    return v, rounds, gsorted


@pytest.mark.gpu
def test_paths_are_live_light_then_heavy(ctx, oracle_mod):
    ctx.set_timeline(True)
    rule, log = HostRule(), []
    L, M, Hs = _scene("L"), _scene("M"), _scene("H")
    v, _, _ = _timeline_pass(ctx, oracle_mod, rule, L, log)
    assert not v["shallow"]                                    # a context's first pass runs deep
    v, rounds, _ = _timeline_pass(ctx, oracle_mod, rule, Hs, log)
    assert v["shallow"] and (rounds > -(-Hs.n_list // 1024)).all()   # the shallow raster met a long list
    v, _, gs = _timeline_pass(ctx, oracle_mod, rule, L, log)
    assert not v["shallow"] and not gs                          # H then L: deep rounds over a short list
    v, _, _ = _timeline_pass(ctx, oracle_mod, rule, L, log)
    assert v["shallow"]                                         # steady-state L
    seq = [_timeline_pass(ctx, oracle_mod, rule, M, log) for _ in range(3)]
    assert seq[0][0]["shallow"] and not seq[1][0]["shallow"]
    assert seq[2][2] and (seq[2][1] * 1024 < M.n_list).any()   # steady-state M: the sorted early exit ran
    print("timeline:", *log, sep="\n  ")


@pytest.mark.gpu
def test_paths_are_live_bin_cap_edges(ctx, oracle_mod):
    """Test 4's sequence under the timeline: 1025 after 1024 (one spilled entry) and 2049 after 2048 (one
    spilled entry under fp.hsort, the tile's hsr range left by the pass before) run every round; the passes
    after them are sorted and end early."""
    ctx.set_timeline(True)
    rule, log = HostRule(), []
    res = [_timeline_pass(ctx, oracle_mod, rule, _list_scene(n), log) for n in BIN_CAP_EDGE_LENGTHS]
    assert [gs for _, _, gs in res] == [False, False, False, True, True, False, True]
    assert not res[2][0]["hsort"] and res[5][0]["hsort"]
    print("timeline:", *log, sep="\n  ")


@pytest.mark.gpu
def test_paths_are_live_parts(ctx, oracle_mod):
    """set_lib_part(64) between two sorted passes: the parts take ranges of list positions of an unsorted
    list, each in whole rounds."""
    ctx.set_timeline(True)
    rule, log = HostRule(), []
    M = _scene("M")
    for _ in range(2):
        _timeline_pass(ctx, oracle_mod, rule, M, log)
    ctx.set_lib_part(64)
    rule.part = 64
    v = rule.predict(M)
    assert not v["hsort"] and not v["shallow"]
    rule.checked_pass(_check(ctx, oracle_mod, M))
    t = ctx.lib_debug_timeline().astype(np.int64)
    F = {k: i for i, k in enumerate(ctx.LIB_TIMELINE_FIELDS)}
    n, k = M.n_list, 16                                          # ceil(n / 64) parts, at most LIB_MAXK = 16
    ends = {n * (j + 1) // k: n * (j + 1) // k - n * j // k for j in range(k)}
    rows = t[t[:, F["mt_items"]] > 256]                         # (a part's mt_items is its end position)
    assert len(rows) >= 1
    for r in rows:
        assert int(r[F["mt_items"]]) in ends, r[F["mt_items"]]
        assert r[F["mt_rounds"]] == -(-ends[int(r[F["mt_items"]])] // 1024)
    ctx.set_lib_part(0)
    rule.part = 0
    _, rounds, gs = _timeline_pass(ctx, oracle_mod, rule, M, log)
    assert gs
    print("timeline:", *log, sep="\n  ")
