"""The scenes of tests/test_canvas_rt_edges.py -- the Canvas render-target raster at its own documented special cases,
which the shaders' scenes of test_canvas_rt_ref.py never reach -- and, on the CPU, what makes them worth running:

  * each scene shows, in the restatement's output alone, the phenomenon it is there for (the assertions fail when the
    special triangle is deleted or the job size changed);
  * the restatement is not the only witness: 'no_colour', 'nonfinite', 'giant' and 'thresholds' are compared on every
    pixel (depth bits, ids, counters) with np_raster, a float32 numpy restatement written again from the cited lines with
    GLM's min / max spelled out; 'small_jobs' is compared, job size by job size, with the oracle's legacy raster;
    'round_boundaries' with the composition of its triangles' solo renders.

Paths are relative to the reference's cpp-folders/src/: "hsm" is hello-render-target/hello_shadow_mapping.cpp, "shs" is
hello-shs-renderer/shs_renderer.hpp.  A scene is (view, light_vp, draws, opts): opts are test_canvas_rt.check_both's
keywords (w, h, sm, tile, and RtFrame's)."""
import dataclasses
import functools

import numpy as np
import pytest

import helpers
import test_canvas_rt_pbr_ref as P
import test_canvas_rt_ref as R
from test_canvas_rt_ref import F, FLT_MAX, NEAR_M, PX_ZTIE, SoupMesh, hair_soup, np_render, ref_render, ref_shadow  # noqa: F401

EYE = np.eye(4, dtype=F).reshape(16)
CLEAR = (20, 20, 25, 255)
NRM = np.array([0, 0, -1] * 3, F)
SMALL_LIGHT = dict(center=(0.0, 0.0, 0.5), dist=5.0, ext=1.5, zf=12.0)   # the light of test_canvas_rt_ref's NEAR_M scenes


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _draw(tris, mvp=EYE, color=(200, 120, 40, 255), normals=None, uvs=None, tex=None, prev=None, model=EYE):
    import shs_gpu
    tris = np.asarray(tris, F).reshape(-1, 9)
    nrm = np.tile(NRM, (tris.shape[0], 1)) if normals is None else normals
    return shs_gpu.RtDraw(SoupMesh(tris, nrm, uvs), model, mvp, mvp if prev is None else prev, color, tex)


def ndc_of_px(p, w, h):
    """Screen pixels [.., 2] -> NDC x, y (the inverse of Canvas::clip_to_screen, shs :823-831)."""
    p = np.asarray(p, np.float64)
    return np.stack([p[..., 0] / (0.5 * (w - 1)) - 1.0, 1.0 - p[..., 1] / (0.5 * (h - 1))], axis=-1)


def render(scene, **over):
    """Both passes through the restatement -> (shadow map, camera planes)."""
    view, lvp, draws, opts = scene
    return R.render_both_ref(view, lvp, draws, **dict(opts, **over))


# ---- 1. small_jobs ---------------------------------------------------------------------------------------------------

SLIVER_W, SLIVER_H, SLIVER_N = 100, 75, 400
JOBS = [(1, 1), (7, 5), (16, 4), (31, 7), (32, 8), (33, 9), (100, 1), (1, 75), (200, 200)]


def scene_small_jobs(tile):
    """400 slivers at 100 x 75 under reference tile jobs smaller than, equal to and misaligned with the 32 x 8 raster
    tile.  A job clamps every sub-triangle's bbox to itself (hsm :806-815 in PASS0, :941-954 in PASS1: bboxmin starts at
    the job's max corner, bboxmax at its min corner, each vertex is folded in under glm::max(tile_min, glm::min(..)) and
    glm::min(tile_max, glm::max(..)), and the loops run over (int) of the result), so it also visits its own edge columns,
    rows and corner pixels for triangles that lie wholly beside it; the slivers' float barycentrics (shs :802-821) pass
    there.  The smaller the job, the more such pixels: the image depends on the job size."""
    mesh = hair_soup(np.random.default_rng(99), SLIVER_W, SLIVER_H, SLIVER_N)
    return EYE, EYE, [_draw(mesh.positions, normals=mesh.normals)], dict(w=SLIVER_W, h=SLIVER_H, sm=(SLIVER_W, SLIVER_H), tile=tile)


def scene_demo_small_jobs(tile):
    """test_canvas_rt_ref.scene_demo (clipped polygons, a texture, the PCF) through small jobs."""
    view, lvp, draws = R.scene_demo()
    return view, lvp, draws, dict(tile=tile)


@functools.lru_cache(maxsize=None)
def small_jobs_planes(tile):
    return render(scene_small_jobs(tile))


def test_small_jobs_change_both_passes():
    sm1, one = small_jobs_planes((SLIVER_W, SLIVER_H))
    seen = {}
    for tile in JOBS:
        sm, out = small_jobs_planes(tile)
        seen[tile] = int((_bits(out["depth"]) != _bits(one["depth"])).sum())
        if tile == (200, 200):
            assert seen[tile] == 0 and np.array_equal(_bits(sm), _bits(sm1))
        else:
            assert seen[tile] >= 100, seen
    assert seen[(1, 1)] > 4 * seen[(7, 5)] > 4 * seen[(32, 8)], seen     # the smaller the job, the more
    assert (_bits(small_jobs_planes((1, 1))[0]) != _bits(sm1)).sum() >= 100
    assert len({seen[t] for t in JOBS}) == len(JOBS), seen               # no two job sizes give the same frame
    # the demo through small jobs still shows what test_canvas_rt_ref's demo is there for
    for tile in ((7, 5), (33, 9)):
        sm, out = render(scene_demo_small_jobs(tile))
        c = out["counters"]
        shaded = out["tri_id"] >= 0
        assert c["polys4"] > 0 and ((out["tri_id"] & 1) == 1)[shaded].any() and (out["texel"] >= 0).sum() > 200
        assert set(np.unique(out["prequant"][..., 3][shaded]).tolist()) == {0.0, 0.25, 0.5, 0.75, 1.0}


def test_small_jobs_are_the_legacy_rasters(oracle_mod):
    """As test_canvas_rt_ref.test_orthographic_frame_is_the_legacy_rasters: w = 1 and view z = NDC z, the slivers turned to
    positive screen area (the legacy raster draws no other) and pre-rotated against the clip loop's {v1, v2, v0} -- then
    coverage and depth bits equal the oracle's legacy raster under the same tile jobs, for every job size."""
    import shs_gpu
    from shs_gpu.scene import Mesh
    w, h, n = SLIVER_W, SLIVER_H, SLIVER_N
    mesh = hair_soup(np.random.default_rng(99), w, h, n)
    pos = mesh.positions.reshape(n, 3, 3).copy()
    sx, sy = (pos[..., 0] + 1.0) * 0.5 * (w - 1), (1.0 - pos[..., 1]) * 0.5 * (h - 1)
    flip = ((sx[:, 1] - sx[:, 0]) * (sy[:, 2] - sy[:, 0]) - (sy[:, 1] - sy[:, 0]) * (sx[:, 2] - sx[:, 0])) <= 0
    pos[flip] = pos[flip][:, [0, 2, 1]]
    nrm = mesh.normals.reshape(n, 3, 3)
    legacy = shs_gpu.Draw(Mesh(pos.reshape(n, 9), nrm.reshape(n, 9)), 3, EYE, EYE, np.array([-0.3, -0.5, 0.8], F), np.array([0, 0, -3], F))
    mine = shs_gpu.RtDraw(SoupMesh(pos[:, [2, 0, 1]].reshape(n, 9), nrm[:, [2, 0, 1]].reshape(n, 9)), EYE, EYE, EYE)
    frames = {}
    for tile in JOBS:
        _, ref_d, _ = oracle_mod.render_legacy(w, h, [legacy], tile=tile)
        out = ref_render(shs_gpu.RtFrame(w, h, EYE, EYE, R.LIGHT_DIR, R.CAM_POS, ref_tile=tile, use_shadow=False), [mine])
        helpers.assert_depth_bitexact(out["depth"][::-1], ref_d)
        frames[tile] = out["depth"]
    assert (_bits(frames[(1, 1)]) != _bits(frames[(200, 200)])).sum() >= 100
    # turned to one winding the slivers ghost less, but every job size below the frame still changes the image
    assert all((_bits(frames[t]) != _bits(frames[(200, 200)])).any() for t in JOBS[:-1])


# ---- 2. no_colour ----------------------------------------------------------------------------------------------------

NC_W, NC_H = 64, 48
NC_FAR = [-0.8, -0.8, 0.6, 0.8, -0.8, 0.6, 0.0, 0.8, 0.6]
NC_NEAR = [-0.5, -0.9, 0.3, 0.9, -0.2, 0.3, -0.2, 0.9, 0.3]
NC_FRONT = [-0.9, 0.1, 0.1, 0.3, 0.0, 0.1, -0.3, 0.7, 0.1]
NC_SCALE = 3e8


def scene_no_colour(with_near=True):
    """hsm :969-980: ZBuffer::test_and_set_depth_screen_space stores the fragment's view z first; only then
    'if (invw_sum <= 1e-8f) continue;' drops the fragment -- its depth stays, colour, velocity and everything else of the
    pixel remain the earlier fragment's (or the clear's).  Draw 1's mvp is 3e8 I: its w is 3e8, 1 / w = 3.3e-9, so every
    one of its fragments is such a fragment, while x / w and the view z (view * model, hsm :615) stay ordinary.
    Draw 0 (far, z = 0.6) lies under part of it, draw 2 (front, z = 0.1) over part of both and wins normally."""
    big = (np.eye(4, dtype=F) * F(NC_SCALE)).reshape(16)
    draws = [_draw([NC_FAR], color=(230, 40, 40, 255))]
    if with_near:
        draws.append(_draw([NC_NEAR], mvp=big, color=(40, 40, 230, 255)))
    draws.append(_draw([NC_FRONT], color=(40, 230, 40, 255)))
    return EYE, R.light(**SMALL_LIGHT), draws, dict(w=NC_W, h=NC_H, sm=40)


def test_no_colour_fragments_keep_their_depth():
    _, out = render(scene_no_colour())
    ids, d = out["tri_id"], out["depth"]
    near = np.abs(d - F(0.3)) < 1e-6
    assert near.sum() > 600
    assert (near & (ids == 0)).sum() > 300                       # the near depth over the far triangle's colour
    bare = near & (ids == -1)
    assert bare.sum() > 100 and (out["color"][bare] == np.array(CLEAR, np.uint8)).all() and not out["velocity"][bare].any()
    assert set(np.unique(ids)) == {-1, 0, 4}                     # draw 1 (id 2) shows nowhere
    front = ids == 4
    assert front.sum() > 100 and (np.abs(d[front] - F(0.1)) < 1e-6).all()
    assert out["counters"] == {"input_tris": 3, "polys3": 3, "polys4": 0, "sub_tris": 3}
    # without draw 1 no pixel has the near depth, and the far triangle's own depth shows under its colour
    _, plain = render(scene_no_colour(with_near=False))
    assert not (np.abs(plain["depth"] - F(0.3)) < 1e-6).any()
    assert ((plain["tri_id"] == 0) & (ids == 0) & near).sum() > 300


# ---- 3. round_boundaries ---------------------------------------------------------------------------------------------

RB_W, RB_H, RB_COLS, RB_ROWS = 144, 90, 18, 15
RB_SIZES = [128, 129, 256, 258]
RB_KINDS = ["tie", "near_first", "far_first"]
# one corner behind the NEAR_M plane: a quad, two sub-triangles (test_canvas_rt_ref.scene_coincident's S)
RB_S = np.array([-0.8, 0.1, 0.5, 0.6, -0.2, 0.7, 0.1, 0.9, -0.5], F)
RB_T = np.array([-0.6, -0.6, 0.6, 0.5, -0.5, 0.3, -0.1, 0.7, 0.8], F)      # unclipped
RB_DZ = np.array([0, 0, 0.05] * 3, F)


def rb_pair_at(n_tris):
    """The triangle index of the pair's first member: the pair straddles camera records 255 | 256 (triangles 127, 128:
    records 254, 255 | 256, 257) where the submission allows, and in the 258-triangle submission camera records
    511 | 512 and shadow-pass records 255 | 256 (triangles 255, 256)."""
    return {128: 126, 129: 127, 256: 127, 258: 255}[n_tris]


def rb_triangles(n_tris, kind):
    """Small disjoint filler triangles, one per cell of an 18 x 15 grid, at z = 0.6 behind NEAR_M (clip = (x, y, z, z + 1)),
    and the pair at rb_pair_at: S, clipped into sub-triangles 2 t and 2 t + 1, and after it
      tie         S again: both of its records tie with the first pair member's on every pixel;
      near_first  S pushed back by 0.05 in z: the later one is farther;
      far_first   the pair the other way round: the later one is nearer.
    A second pair of unclipped triangles (T, T again) sits at the very end of the submission."""
    k = np.arange(n_tris)
    cx = (k % RB_COLS + 0.5) / RB_COLS * 2.0 - 1.0
    cy = (k // RB_COLS + 0.5) / RB_ROWS * 2.0 - 1.0
    dx, dy = 0.6 / RB_COLS, 0.6 / RB_ROWS
    tris = np.empty((n_tris, 3, 3), F)
    tris[:, 0, :2] = np.stack([cx - dx, cy - dy], 1)
    tris[:, 1, :2] = np.stack([cx + dx, cy - dy], 1)
    tris[:, 2, :2] = np.stack([cx, cy + dy], 1)
    tris[..., :2] *= 1.6
    tris[..., 2] = 0.6
    tris = tris.reshape(n_tris, 9)
    a = rb_pair_at(n_tris)
    first, second = {"tie": (RB_S, RB_S), "near_first": (RB_S, RB_S + RB_DZ), "far_first": (RB_S + RB_DZ, RB_S)}[kind]
    tris[a], tris[a + 1] = first, second
    if a + 1 < n_tris - 2:
        tris[n_tris - 2] = tris[n_tris - 1] = RB_T
    return tris


def scene_round_boundaries(n_tris, kind):
    """The raster walks the submission in rounds of 256 records; the reference walks it in order (hsm :1320-1411 and the
    camera pass after it), ZBuffer::test_and_set_depth_screen_space (shs :671-675) taking a fragment only when
    'z < depth': of equal depths the first wins, whichever round either lies in."""
    return EYE, R.light(**SMALL_LIGHT), [_draw(rb_triangles(n_tris, kind), mvp=NEAR_M, color=(230, 40, 40, 255))], \
        dict(w=RB_W, h=RB_H, sm=72)


def _compose_solo(scene, special):
    """The ids of the frame composed from solo renders: the triangles `special` each alone, the rest together, merged in
    submission order under the strict '<'."""
    view, lvp, draws, opts = scene
    tris = draws[0].mesh.positions
    far = np.array([0, 0, -5.0] * 3, F)               # behind the plane: clipped away, but keeps its place in the order
    depth = np.full((opts["h"], opts["w"]), FLT_MAX, F)
    ids = np.full(depth.shape, -1, np.int32)
    rest = tris.copy()
    rest[special] = far
    layers = [(0, rest)]
    for s in special:
        solo = np.tile(far, (tris.shape[0], 1))
        solo[s] = tris[s]
        layers.append((s, solo))
    outs = []
    for first, t in layers:
        frame = R._frame(view, lvp, opts["w"], opts["h"], use_shadow=False)
        outs.append((first, ref_render(frame, [dataclasses.replace(draws[0], mesh=SoupMesh(t))])))
    # the fillers are disjoint and lie among themselves in order; the specials follow in submission order
    for first, o in sorted(outs, key=lambda e: e[0] if e[0] in special else -1):
        win = o["depth"] < depth
        depth[win], ids[win] = o["depth"][win], o["tri_id"][win]
    return depth, ids


@pytest.mark.parametrize("kind", RB_KINDS)
@pytest.mark.parametrize("n_tris", RB_SIZES)
def test_round_boundaries_show_the_expected_winners(n_tris, kind):
    scene = scene_round_boundaries(n_tris, kind)
    sm, out = render(scene)
    ids, a = out["tri_id"], rb_pair_at(n_tris)
    c = out["counters"]
    assert c["input_tris"] == n_tris and c["polys4"] == 2 and c["sub_tris"] == n_tris + 2
    assert 2 * n_tris in (256, 258, 512, 516) and (2 * a + 1) % 256 in (253, 255)
    first, second = {2 * a, 2 * a + 1}, {2 * a + 2, 2 * a + 3}
    shown = set(np.unique(ids).tolist())
    tie = (out["flags"] & PX_ZTIE) != 0
    if kind == "tie":
        assert first <= shown and not (second & shown)
        assert (tie & np.isin(ids, list(first))).sum() > 500 and tie[ids == 2 * a + 1].all()
    else:
        assert first <= shown and second <= shown
        n_first, n_second = np.isin(ids, list(first)).sum(), np.isin(ids, list(second)).sum()
        assert (n_first > 4 * n_second) if kind == "near_first" else (n_second > 4 * n_first), (n_first, n_second)
    special = [a, a + 1] + ([n_tris - 2, n_tris - 1] if a + 1 < n_tris - 2 else [])
    if len(special) == 4:                                                    # T twice at the end: the first shows
        assert 2 * (n_tris - 2) in shown and 2 * (n_tris - 1) not in shown and tie[ids == 2 * (n_tris - 2)].all()
    depth, want = _compose_solo(scene, special)
    helpers.assert_depth_bitexact(out["depth"], depth)
    assert np.array_equal(ids, want)
    assert len(shown) > n_tris // 2                                          # the fillers show too
    assert (sm < FLT_MAX).sum() > 300


# ---- 4. nonfinite ----------------------------------------------------------------------------------------------------

NF_W, NF_H, NF_OK = 64, 48, 50
NAN, INF = float("nan"), float("inf")


def _small_triangles(rng, n, w, h, lo=-0.3, hi=0.8):
    """n triangles of circumradius 10^lo .. 10^hi px around random points of the frame, z in (0.1, 0.9)."""
    c = rng.uniform([0, 0], [w, h], size=(n, 1, 2))
    size = 10 ** rng.uniform(lo, hi, size=(n, 1))
    ang = rng.uniform(0, 2 * np.pi, size=(n, 1)) + np.array([0, 2.1, 4.2])
    p = c + size[..., None] * np.stack([np.cos(ang), np.sin(ang)], -1)
    out = np.empty((n, 3, 3), F)
    out[..., :2] = ndc_of_px(p, w, h)
    out[..., 2] = rng.uniform(0.1, 0.9, size=(n, 3))
    return out.reshape(n, 9)


def nonfinite_triangles():
    """50 ordinary triangles, then five whose position has, in turn: NaN in x of corner 0, NaN in z of corner 1, +inf in x
    of corner 1, -inf in y of corner 2, NaN everywhere."""
    rng = np.random.default_rng(17)
    ok = _small_triangles(rng, NF_OK, NF_W, NF_H, 0.3, 1.0)
    bad = _small_triangles(rng, 5, NF_W, NF_H, 0.8, 1.2)
    bad[0, 0] = NAN
    bad[1, 5] = NAN
    bad[2, 3] = INF
    bad[3, 7] = -INF
    bad[4, :] = NAN
    return np.concatenate([ok, bad])


def scene_nonfinite():
    """A non-finite position component makes the corner's whole clip position NaN or infinite with w NaN (0 * inf and
    0 * NaN in the mat4 * vec4 of vertex_shader_full, hsm :602-620).  'inside' (hsm :881-883: w > 1e-6 && z >= 0) is false
    for it, so a triangle with one such corner leaves clip_poly_near_z (hsm :877-913) with four vertices, two of them
    intersect()'s output at t = NaN (hsm :885-893: fabs(NaN) < 1e-8 is false, clampf keeps a NaN); both fan
    sub-triangles hold a NaN corner, pass 'w <= 1e-6f' (false for NaN, hsm :936) and 'fabs(area) < 1e-8f' (false, hsm :959),
    and reach the pixel loops over the bbox of their finite corners (glm::min / max keep the other operand, hsm :949-953),
    where NaN barycentrics pass all three '< 0' tests and the NaN depth fails 'z < depth'.  All nine components NaN: no
    corner inside, no polygon.  The same menu through the identity and through NEAR_M."""
    tris = nonfinite_triangles()
    draws = [_draw(tris, color=(230, 40, 40, 255)), _draw(tris[::-1].copy(), mvp=NEAR_M, color=(40, 40, 230, 255))]
    return EYE, R.light(**SMALL_LIGHT), draws, dict(w=NF_W, h=NF_H, sm=40)


NF_COUNTERS = {"input_tris": 2 * (NF_OK + 5), "polys3": 2 * NF_OK, "polys4": 2 * 4, "sub_tris": 2 * NF_OK + 2 * 4 * 2}


def test_nonfinite_positions_change_the_counters_and_nothing_else():
    sm, out = render(scene_nonfinite())
    assert out["counters"] == NF_COUNTERS
    for k in ("depth", "velocity", "prequant", "color"):
        assert np.isfinite(out[k].astype(np.float64)).all(), k
    assert np.isfinite(sm).all()
    shown = set(np.unique(out["tri_id"]).tolist()) - {-1}
    assert len(shown) > 60 and all(i % 2 == 0 for i in shown)
    bad = set(range(2 * NF_OK, 2 * (NF_OK + 5))) | set(range(2 * (NF_OK + 5), 2 * (NF_OK + 5) + 10))   # draw 1 holds them first
    assert not (shown & bad) and (sm < FLT_MAX).sum() > 100
    # the finite triangles' frame is the frame
    view, lvp, draws, opts = scene_nonfinite()
    clean = [dataclasses.replace(d, mesh=SoupMesh(np.where(np.isfinite(d.mesh.positions).all(1, keepdims=True), d.mesh.positions,
                                                            np.array([0, 0, -5.0] * 3, F)))) for d in draws]
    sm2, out2 = R.render_both_ref(view, lvp, clean, **opts)
    assert np.array_equal(out2["tri_id"], out["tri_id"]) and np.array_equal(_bits(out2["depth"]), _bits(out["depth"]))
    assert out2["counters"]["polys4"] == 0


def scene_nonfinite_attributes():
    """NaN and infinite normals and UVs on triangles that are shown, textured.  A NaN normal makes the colour NaN before
    the truncation ((uint8_t) of a NaN float is 0 in the reference's x86-64 build), a NaN uv makes saturate's output NaN
    and std::lround's (int) 0 (shs :367-377); an infinite uv saturates to texel 0 or the last."""
    rng = np.random.default_rng(23)
    n = 24
    tris = _small_triangles(rng, n, NF_W, NF_H, 0.7, 1.1)
    nrm = rng.normal(size=(n, 9)).astype(F)
    uvs = rng.uniform(-0.2, 1.2, size=(n, 6)).astype(F)
    nrm[0, 0] = NAN
    nrm[1, 4] = INF
    nrm[2, :] = NAN
    nrm[3, 8] = -INF
    uvs[4, 0] = NAN
    uvs[5, 3] = INF
    uvs[6, 4] = -INF
    uvs[7, :] = NAN
    nrm[8, 2], uvs[8, 5] = NAN, NAN
    return EYE, R.light(**SMALL_LIGHT), [_draw(tris, normals=nrm, uvs=uvs, tex=R.TEX)], dict(w=NF_W, h=NF_H, sm=40)


def test_nonfinite_attributes_reach_the_planes():
    _, out = render(scene_nonfinite_attributes())
    pq, ids = out["prequant"], out["tri_id"]
    nan = np.isnan(pq[..., :3]).any(-1)
    assert nan.sum() > 100 and (out["color"][nan][:, :3] == 0).all() and (out["color"][nan][:, 3] == 255).all()
    assert {0, 2, 4, 6, 16} <= set(np.unique(ids[nan]).tolist())                    # the NaN and inf normals
    assert np.isfinite(out["depth"]).all() and np.isfinite(out["velocity"]).all()
    for t in (4, 5, 6, 7):                                                         # the bad uvs: a colour, a texel
        px = ids == 2 * t
        assert px.sum() > 20 and not nan[px].any() and (out["texel"][px] >= 0).all()
    tw = R.TEX.rgba.shape[1]
    assert (out["texel"][ids == 14] == 0).all()                                    # all uvs NaN: texel (0, 0)
    assert ((out["texel"][ids == 8] % tw) == 0).all()                              # u NaN at every pixel: column 0


# ---- 5. giant --------------------------------------------------------------------------------------------------------

G_W, G_H, G_N = 64, 48, 40
G_FIXED = (1e12, 1e19, 1e30)


def giant_scales():
    return 10 ** np.random.default_rng(31).uniform(3, 8.5, size=G_N)


def scene_giant():
    """Triangles whose NDC corners are scaled by 1e3 .. 3e8 and by 1e12, 1e19 and 1e30, through the identity.  Their
    screen coordinates (shs :823-831) reach 1e10 px and beyond: barycentric_coordinate's products (shs :802-821) lose
    their precision, then overflow -- d00 * d11 - d01 * d01 becomes inf - inf, every barycentric NaN and the depth with it
    -- so up to a scale of about 1e7 a giant still fills the frame and above it draws nothing; the bbox is the tile job
    (hsm :941-954) either way.  A few ordinary triangles lie in front."""
    scales = np.concatenate([giant_scales(), G_FIXED])
    rng2 = np.random.default_rng(32)
    tris = np.empty((len(scales), 3, 3), np.float64)
    for i, s in enumerate(scales):
        if i % 4 == 0:      # around the frame: it fills it, at a nearly constant depth
            ang = rng2.uniform(0, 2 * np.pi) + np.array([0, 2.1, 4.2]) + rng2.uniform(-0.3, 0.3, 3)
            tris[i, :, :2] = (np.stack([np.cos(ang), np.sin(ang)], 1) + rng2.uniform(-0.2, 0.2, 2)) * s
        else:               # a wedge: one corner in the frame, the other two far away
            a0, da = rng2.uniform(0, 2 * np.pi), rng2.uniform(0.2, 1.2)
            tris[i, 0, :2] = rng2.uniform(-0.9, 0.9, 2)
            tris[i, 1:, :2] = np.array([[np.cos(a0), np.sin(a0)], [np.cos(a0 + da), np.sin(a0 + da)]]) * s
        tris[i, :, 2] = rng2.uniform(0.2, 0.9, 3)
    front = _small_triangles(np.random.default_rng(33), 6, G_W, G_H, 0.7, 1.0).reshape(6, 3, 3)
    front[..., 2] = 0.05
    draws = [_draw(tris.astype(F).reshape(-1, 9), color=(230, 40, 40, 255)), _draw(front.reshape(6, 9), color=(40, 230, 40, 255))]
    return EYE, EYE, draws, dict(w=G_W, h=G_H, sm=(50, 40))


def test_giants_fill_the_frame_until_their_products_overflow():
    sm, out = render(scene_giant())
    ids = out["tri_id"]
    giants = ids[(ids >= 0) & (ids < 2 * (G_N + 3))] // 2
    shown = set(np.unique(giants).tolist())
    assert len(shown) >= 5, shown
    silent = [i for i in range(G_N) if i not in shown]
    assert silent and not (shown & {G_N, G_N + 1, G_N + 2})                  # 1e12, 1e19, 1e30 draw nothing
    under = (ids >= 0) & (ids < 2 * (G_N + 3))
    assert under.sum() > 0.8 * G_W * G_H and len(np.unique(out["depth"][under])) > 100
    assert (ids >= 2 * (G_N + 3)).sum() > 50                                 # the ordinary ones in front
    assert out["counters"]["polys3"] == G_N + 3 + 6 and np.isfinite(out["depth"]).all()
    assert (sm < FLT_MAX).sum() > 0.8 * 50 * 40 and np.isfinite(sm).all()
    # a giant that shows nothing alone, although it is nearer than what shows at the pixels it would cover
    view, lvp, draws, opts = scene_giant()
    big = int(np.argmax(giant_scales()))
    assert big in silent
    solo = ref_render(R._frame(view, lvp, G_W, G_H, use_shadow=False), [dataclasses.replace(draws[0], mesh=SoupMesh(draws[0].mesh.positions[big]))])
    assert (solo["tri_id"] == -1).all() and solo["counters"]["sub_tris"] == 1


# ---- 6. thresholds ---------------------------------------------------------------------------------------------------

TH_W, TH_H, TH_N = 64, 48, 2000
TH_WS = (9e-7, 1e-6, 1.1e-6, 1e-5)
# clip = (x, y, 0.5, z): w is the corner's z
W_IS_Z = np.zeros((4, 4), F)
W_IS_Z[0, 0] = W_IS_Z[1, 1] = 1.0
W_IS_Z[2, 3] = 0.5
W_IS_Z[3, 2] = 1.0
W_IS_Z = np.ascontiguousarray(W_IS_Z.T).reshape(16)
# the light: clip = (x, y, 0.5 z, z), so ndc z is 0.5 wherever w is not dropped
LIGHT_W_IS_Z = np.zeros((4, 4), F)
LIGHT_W_IS_Z[0, 0] = LIGHT_W_IS_Z[1, 1] = LIGHT_W_IS_Z[3, 2] = 1.0
LIGHT_W_IS_Z[2, 2] = 0.5
LIGHT_W_IS_Z = np.ascontiguousarray(LIGHT_W_IS_Z.T).reshape(16)


def tiny_triangles():
    rng = np.random.default_rng(5)
    c = rng.integers([0, 0], [TH_W, TH_H], size=(TH_N, 2)) + 0.5
    size = 10 ** rng.uniform(-3.5, 0.3, size=TH_N)
    c = c + rng.normal(size=(TH_N, 2)) * size[:, None] * 0.1
    ang = rng.uniform(0, 2 * np.pi, size=(TH_N, 1)) + np.array([0, 2.1, 4.2])
    p = c[:, None, :] + size[:, None, None] * np.stack([np.cos(ang), np.sin(ang)], -1)
    out = np.empty((TH_N, 3, 3), F)
    out[..., :2] = ndc_of_px(p, TH_W, TH_H)
    out[..., 2] = rng.uniform(0.1, 0.9, size=(TH_N, 3))
    return out.reshape(TH_N, 9), size


def w_triangles():
    """Per w of TH_WS a triangle whose corner 0 has that w (x and y scaled by it, so it stays on the screen) and whose
    other corners have w = 0.5; then per w a triangle with all three corners at it."""
    tris = []
    for i, wv in enumerate(TH_WS):
        x0 = -0.8 + 0.4 * i
        tris.append([x0 * wv, 0.8 * wv, wv, (x0 + 0.3) * 0.5, 0.1 * 0.5, 0.5, (x0 - 0.05) * 0.5, 0.2 * 0.5, 0.5])
    for i, wv in enumerate(TH_WS):
        x0 = -0.8 + 0.4 * i
        tris.append([x0 * wv, -0.2 * wv, wv, (x0 + 0.3) * wv, -0.8 * wv, wv, (x0 - 0.05) * wv, -0.9 * wv, wv])
    return np.array(tris, F)


def scene_thresholds():
    """2000 triangles of circumradius 10^-3.5 .. 2 px about pixel centres: the smallest fall under 'fabs(area) < 1e-8f'
    (hsm :958-959) or under barycentric_coordinate's 'std::abs(denom) < 1e-5' (shs :815-816, a double comparison, every
    barycentric -1), the next ones cover their pixel centre or just miss it.  And the w tests: 'inside' needs w > 1e-6
    (hsm :881-883), a sub-triangle is dropped when a corner's w <= 1e-6f (hsm :936); 9e-7 and 1e-6 are out, 1.1e-6 and 1e-5
    are in.  A corner that is out is cut at t = 0 (the clip z is constant: fabs(bz - az) < 1e-8, hsm :890), so the cut
    is the outside corner itself and the w test drops both fan sub-triangles.  (area_triangles holds the ones around
    1e-8 px^2.)  The light's w is the world z as well: PASS0 drops a caster when fabs(w) < 1e-6f (hsm :802) -- 9e-7 is
    out, and 1e-6, out in the camera pass, is in."""
    tiny, _ = tiny_triangles()
    draws = [_draw(tiny), _draw(w_triangles(), mvp=W_IS_Z, color=(40, 40, 230, 255)), _draw(area_triangles(), color=(40, 230, 40, 255))]
    return EYE, LIGHT_W_IS_Z, draws, dict(w=TH_W, h=TH_H, sm=40)


TH_AREA_N = 60


def area_triangles():
    """60 triangles of circumradius 10^-4.8 .. 10^-3.6 px in the frame's first pixel, where a float's ulp is 6e-8 px: their
    areas lie on both sides of 1e-8 px^2 (the 2000 above sit at coordinates whose ulp is 4e-6 px: their areas are
    0 or far above it)."""
    rng = np.random.default_rng(7)
    c = rng.uniform(0.3, 0.7, size=(TH_AREA_N, 1, 2))
    size = 10 ** rng.uniform(-4.8, -3.6, size=(TH_AREA_N, 1))
    ang = rng.uniform(0, 2 * np.pi, size=(TH_AREA_N, 1)) + np.array([0, 2.1, 4.2])
    p = c + size[..., None] * np.stack([np.cos(ang), np.sin(ang)], -1)
    out = np.empty((TH_AREA_N, 3, 3), F)
    out[..., :2] = ndc_of_px(p, TH_W, TH_H)
    out[..., 2] = 0.5
    return out.reshape(TH_AREA_N, 9)


def screen_geometry(tris, w, h):
    """|area| (hsm :958) and |denom| (shs :802-815) of triangles through the identity, in the reference's float32 order."""
    t = np.asarray(tris, F).reshape(-1, 3, 3)
    sx = ((t[..., 0] / F(1) + F(1)) * F(0.5)) * F(w - 1)
    sy = ((F(1) - t[..., 1] / F(1)) * F(0.5)) * F(h - 1)
    assert sx.dtype == F
    # the clip loop turns {v0, v1, v2} into {v1, v2, v0}
    sx, sy = sx[:, [1, 2, 0]], sy[:, [1, 2, 0]]
    v0x, v0y, v1x, v1y = sx[:, 1] - sx[:, 0], sy[:, 1] - sy[:, 0], sx[:, 2] - sx[:, 0], sy[:, 2] - sy[:, 0]
    area = np.abs(v0x * v1y - v0y * v1x)
    d00, d01, d11 = v0x * v0x + v0y * v0y, v0x * v1x + v0y * v1y, v1x * v1x + v1y * v1y
    return area, np.abs(d00 * d11 - d01 * d01).astype(np.float64)


def test_thresholds_split_the_tiny_and_the_small_w():
    _, out = render(scene_thresholds())
    tiny, size = tiny_triangles()
    ids, c = out["tri_id"], out["counters"]
    shown = np.unique(ids[(ids >= 0) & (ids < 2 * TH_N)]) // 2
    assert 300 < len(shown) < TH_N - 300
    assert size[shown].min() < 0.1 and (size < 10 ** -3.0).sum() > 100              # the smallest that show: |denom| >= 1e-5
    # the area test, from the float32 screen coordinates: sub_tris counts exactly the sub-triangles that pass it
    area, den = screen_geometry(tiny, TH_W, TH_H)
    area2, den2 = screen_geometry(area_triangles(), TH_W, TH_H)
    n_w = 4                                                                   # of w_triangles: the four with w > 1e-6
    assert 10 < (area2 < F(1e-8)).sum() < TH_AREA_N - 10 and (den2 < 1e-5).all()
    assert c["sub_tris"] == int((area >= F(1e-8)).sum()) + n_w + int((area2 >= F(1e-8)).sum()), c
    # denom: triangles that pass the area test and still show nothing, whatever they cover
    small = (area >= F(1e-8)) & (den < 1e-5)
    assert small.sum() > 100 and not np.isin(np.nonzero(small)[0], shown).any()
    assert np.isin(np.nonzero(den >= 1e-5)[0], shown).sum() > 300 and (ids < 2 * (TH_N + 8)).all()
    # the w cases: corner 0 at 9e-7 and 1e-6 -> a quad whose sub-triangles both fail the w test; at 1.1e-6 and 1e-5 ->
    # a triangle that shows.  All corners at 9e-7 or 1e-6 -> nothing inside; at 1.1e-6 or 1e-5 -> a triangle that shows.
    assert c["polys4"] == 2 and c["polys3"] == TH_N + 4 + TH_AREA_N and c["input_tris"] == TH_N + 8 + TH_AREA_N
    w_ids = set(np.unique(ids[ids >= 2 * TH_N]).tolist())
    assert w_ids == {2 * (TH_N + k) for k in (2, 3, 6, 7)}, w_ids
    # PASS0: fabs(w) < 1e-6f drops the casters with a corner at 9e-7 and no other
    covered = [int((ref_shadow(40, LIGHT_W_IS_Z, [_draw(t)]) < FLT_MAX).sum()) for t in w_triangles()]
    assert [n > 0 for n in covered] == [False, True, True, True, False, True, True, True], covered


# ---- 7. perspective_light --------------------------------------------------------------------------------------------

PL_EYE, PL_AT = (2.0, 5.0, -3.0), (-1.0, 0.5, 4.0)


def perspective_light():
    """perspective * look_at with z remapped to [0, 1]: clip w is the light-space depth, not 1."""
    from shs_gpu import lib_path
    proj = lib_path.perspective_lh_no(float(np.radians(80.0)), 1.0, 1.0, 40.0)
    remap = np.eye(4, dtype=F)
    remap[2, 2], remap[2, 3] = 0.5, 0.5                                      # z' = 0.5 z + 0.5 w
    remap = np.ascontiguousarray(remap.T).reshape(16)
    return R._mul(R._mul(remap, proj), lib_path.look_at_lh(PL_EYE, PL_AT))


def scene_perspective_light(pcf=True):
    """The demo's draws under a light whose clip w varies.  shadow_vertex_shader / clip_to_shadow_screen (hsm :761-783)
    divide by it without clipping -- PASS0 only drops a triangle when fabs(w) < 1e-6 (hsm :802) -- so the floor's
    triangles behind the light's w = 0 plane are projected as they are, mirrored and far outside the map; the camera
    pass's shadow_uvz_from_world (hsm :628-648) divides the receiver's position the same way."""
    view, _, draws = R.scene_demo()
    return view, perspective_light(), draws, dict(pcf=pcf)


def test_perspective_light_divides_by_w():
    view, lvp, draws, _ = scene_perspective_light()
    cw = []
    for d in draws:
        lm = R._mul(lvp, d.model)
        cw += [R._m4(lm, p)[3] for p in d.mesh.positions.reshape(-1, 3)[::7]]
    cw = np.array(cw)
    assert (cw < 0).sum() > 5 and (cw > 1).sum() > 100 and len(np.unique(np.round(cw, 2))) > 50
    floor_w = np.array([R._m4(R._mul(lvp, draws[0].model), p)[3] for p in draws[0].mesh.positions.reshape(-1, 3)]).reshape(-1, 3)
    assert ((floor_w < 0).any(1) & (floor_w > 0).any(1)).sum() >= 3          # floor triangles that cross w = 0
    sm, out = render(scene_perspective_light())
    shaded = out["tri_id"] >= 0
    assert 1000 < (sm < FLT_MAX).sum() and len(np.unique(sm)) > 500
    assert set(np.unique(out["prequant"][..., 3][shaded]).tolist()) == {0.0, 0.25, 0.5, 0.75, 1.0}
    _, nop = render(scene_perspective_light(pcf=False))
    fac = nop["prequant"][..., 3][nop["tri_id"] >= 0]
    assert set(np.unique(fac).tolist()) == {0.0, 1.0} and (fac == 0).sum() > 200
    # an orthographic light of the same direction gives another map and other factors: w matters
    _, ortho = R.render_both_ref(view, R.light(), draws)
    assert (ortho["prequant"][..., 3] != out["prequant"][..., 3]).sum() > 500


# ---- the scenes by name, for the GPU tests ---------------------------------------------------------------------------

def shading_scene(name):
    """The two scenes that also run through shadings 1, 2 and 3."""
    return {"no_colour": scene_no_colour, "round_boundaries": lambda: scene_round_boundaries(129, "tie")}[name]()


SHADING_NAMES = ["no_colour", "round_boundaries"]


def edge_materials(draws, which):
    """test_canvas_rt_pbr_ref.edge_scene's materials over these draws."""
    mat = P.ROUGH_DIELECTRIC if which == "rough" else P.SMOOTH_METAL
    return [P.material(P.TURNS[which][i % 3], **mat) for i in range(len(draws))]


@pytest.mark.parametrize("name", SHADING_NAMES)
def test_other_shadings_restatements_raster_alike(name):
    """The soft, PBR and PBR-under-PCSS restatements carry their own copies of the camera raster's loops: on these two
    scenes their depth, ids and counters are test_canvas_rt_ref's, so the rules hold in every reference the GPU meets."""
    import test_canvas_rt_pbr_soft_ref as Q
    import test_canvas_rt_soft_ref as S
    view, lvp, draws, opts = shading_scene(name)
    w, h = opts["w"], opts["h"]
    sm = ref_shadow(opts["sm"], lvp, draws)
    hard = ref_render(R._frame(view, lvp, w, h), draws, sm)
    mats = edge_materials(draws, "rough")
    others = [S.ref_render_soft(S.soft_frame(view, lvp, w, h), draws, sm),
              P.ref_render_pbr(P.pbr_frame(view, lvp, w, h), draws, mats, sm, P.make_ibl()),
              Q.ref_render_pbr_soft(Q.pbr_soft_frame(view, lvp, w, h), draws, mats, sm, P.make_ibl())]
    for o in others:
        assert np.array_equal(_bits(o["depth"]), _bits(hard["depth"])) and np.array_equal(o["tri_id"], hard["tri_id"])
        assert o["counters"] == hard["counters"]


# ---- the restatement against numpy -----------------------------------------------------------------------------------

def g_min(x, y):
    """glm::min(x, y) = (y < x) ? y : x -- a NaN y is dropped, a NaN x kept; np.minimum is another function."""
    return y if y < x else x


def g_max(x, y):
    """glm::max(x, y) = (x < y) ? y : x"""
    return y if x < y else x


def int_x86(f):
    """(int)f of the reference's x86-64 build (cvttss2si): INT_MIN for a NaN and out of range."""
    return int(f) if np.isfinite(f) and -2147483648.0 <= f < 2147483648.0 else -2147483648


def np_raster(frame, draws):
    """hsm :854-1022 up to the depth test and the invw_sum rule, one tile job (the whole frame), in float32 numpy, a
    sub-triangle's pixels at once: (depth, ids, counters).  Vertices and the clip are test_canvas_rt_ref's _m4 and
    _np_clip; the bbox, the barycentrics, the depth test and the counters are written here from the cited lines."""
    Wd, Hd = frame.width, frame.height
    depth = np.full((Hd, Wd), FLT_MAX, F)
    ids = np.full((Hd, Wd), -1, np.int32)
    cnt = {"input_tris": 0, "polys3": 0, "polys4": 0, "sub_tris": 0}
    t = 0

    def screen(p):
        return F(F(F(F(p[0] / p[3]) + F(1)) * F(0.5)) * F(Wd - 1)), F(F(F(F(1) - F(p[1] / p[3])) * F(0.5)) * F(Hd - 1))
    with np.errstate(all="ignore"):
        for d in draws:
            vm = R._mul(frame.view, d.model)
            for k in range(d.mesh.positions.shape[0]):
                vs = []
                for c in range(3):
                    p = d.mesh.positions[k, 3 * c:3 * c + 3]
                    vs.append({"p": np.array(R._m4(d.mvp, p), F), "vz": np.array([R._m4(vm, p)[2]], F)})
                poly = R._np_clip(vs)
                cnt["input_tris"] += 1
                cnt["polys3"] += len(poly) == 3
                cnt["polys4"] += len(poly) == 4
                for ti in range(1, len(poly) - 1):
                    tv = [poly[0], poly[ti], poly[ti + 1]]
                    if any(v["p"][3] <= F(1e-6) for v in tv):                       # hsm :936
                        continue
                    s = [screen(v["p"]) for v in tv]
                    # hsm :941-954: the bbox from the job's far corners, NaN corners dropped by glm::min / max
                    bmin, bmax = [F(Wd - 1), F(Hd - 1)], [F(0), F(0)]
                    for q in s:
                        for a, (lo, hi) in enumerate(((F(0), F(Wd - 1)), (F(0), F(Hd - 1)))):
                            bmin[a] = g_max(lo, g_min(bmin[a], q[a]))
                            bmax[a] = g_min(hi, g_max(bmax[a], q[a]))
                    v0 = (F(s[1][0] - s[0][0]), F(s[1][1] - s[0][1]))
                    v1 = (F(s[2][0] - s[0][0]), F(s[2][1] - s[0][1]))
                    area = F(F(v0[0] * v1[1]) - F(v0[1] * v1[0]))
                    if not abs(area) < F(1e-8):
                        cnt["sub_tris"] += 1
                    if bmin[0] > bmax[0] or bmin[1] > bmax[1] or abs(area) < F(1e-8):
                        continue
                    x0, x1, y0, y1 = int_x86(bmin[0]), int_x86(bmax[0]), int_x86(bmin[1]), int_x86(bmax[1])
                    if x1 < x0 or y1 < y0:
                        continue
                    d00 = F(F(v0[0] * v0[0]) + F(v0[1] * v0[1]))
                    d01 = F(F(v0[0] * v1[0]) + F(v0[1] * v1[1]))
                    d11 = F(F(v1[0] * v1[0]) + F(v1[1] * v1[1]))
                    den = F(F(d00 * d11) - F(d01 * d01))
                    if abs(float(den)) < 1e-5:                                      # shs :815-816: (-1, -1, -1)
                        continue
                    iw = [F(0) if abs(v["p"][3]) < F(1e-6) else F(F(1) / v["p"][3]) for v in tv]
                    px, py = np.meshgrid(np.arange(x0, x1 + 1), np.arange(y0, y1 + 1))
                    vx = (px.astype(F) + F(0.5)) - s[0][0]
                    vy = (py.astype(F) + F(0.5)) - s[0][1]
                    d20 = vx * v0[0] + vy * v0[1]
                    d21 = vx * v1[0] + vy * v1[1]
                    bv = (d11 * d20 - d01 * d21) / den
                    bw = (d00 * d21 - d01 * d20) / den
                    bu = (F(1) - bv) - bw
                    assert bu.dtype == F and d20.dtype == F
                    ok = ~((bu < 0) | (bv < 0) | (bw < 0))
                    vz = (bu * tv[0]["vz"][0] + bv * tv[1]["vz"][0]) + bw * tv[2]["vz"][0]
                    yc = Hd - 1 - py
                    win = ok & (vz < depth[yc, px])                                 # shs :671-675
                    depth[yc[win], px[win]] = vz[win]
                    isum = (bu * iw[0] + bv * iw[1]) + bw * iw[2]
                    col = win & ~(isum <= F(1e-8))                                  # hsm :980
                    ids[yc[col], px[col]] = 2 * t + ti - 1
                t += 1
    return depth, ids, {k: int(v) for k, v in cnt.items()}


PINNED = {"no_colour": scene_no_colour, "nonfinite": scene_nonfinite, "giant": scene_giant, "thresholds": scene_thresholds}


@pytest.mark.parametrize("name", list(PINNED))
def test_raster_equals_numpy_restatement(name):
    view, lvp, draws, opts = PINNED[name]()
    w, h = opts["w"], opts["h"]
    frame = R._frame(view, lvp, w, h, (w, h), use_shadow=False)
    out = ref_render(frame, draws)
    depth, ids, cnt = np_raster(frame, draws)
    helpers.assert_depth_bitexact(out["depth"], depth)
    bad = np.argwhere(out["tri_id"] != ids)
    assert bad.size == 0, f"{len(bad)} ids differ, first {bad[:4].tolist()}"
    assert out["counters"] == cnt
    assert (ids >= 0).sum() > 200


def test_np_raster_equals_np_render():
    """The vectorised restatement against test_canvas_rt_ref's per-pixel one, on that file's clipped quad and triangle."""
    import shs_gpu
    mesh = R.near_mesh()
    draws = [shs_gpu.RtDraw(SoupMesh(mesh.positions[:2], mesh.normals[:2], mesh.uvs[:2]), EYE, NEAR_M, NEAR_M, (210, 180, 90, 255), R.TEX)]
    frame = shs_gpu.RtFrame(48, 36, EYE, EYE, R.LIGHT_DIR, R.CAM_POS, ref_tile=(48, 36), use_shadow=False)
    depth, ids, _, _ = np_render(frame, draws)
    d2, i2, cnt = np_raster(frame, draws)
    assert np.array_equal(_bits(depth), _bits(d2)) and np.array_equal(ids, i2)
    assert cnt == {"input_tris": 2, "polys3": 1, "polys4": 1, "sub_tris": 3}
