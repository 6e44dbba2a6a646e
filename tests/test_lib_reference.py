"""The library-path oracle against the COMPILED REFERENCE, bit for bit (CPU).

oracle/_ref/libshs_ref_lib.so is the reference library's own rasterize_mesh, builtin programs, texture
sampler, PCF, PassTonemap and PassMotionBlur, compiled over a GLM stand-in (oracle/ref_lib.cpp,
oracle/glm_standin/).  Both sides are the same IEEE single-precision operations, built by the same compiler
without contraction, calling the same libm: every 32-bit word and every byte must be equal, no tolerance.
GLM itself stays unpinned (the stand-in restates it).

Every rendered case also asserts that it covers pixels and rasterises triangles, and the cases about
clipping / shadowing that clipping / shadowing happened."""
import copy

import numpy as np
import pytest

import lib_ref_cases as cases
from test_lib_parity import _camera, _clip_soup
from test_post import MB_CASES

_WORDS = {"cases": 0, "words": 0}     # tally, printed by test_zz_tally (run with -s to read it)


@pytest.fixture(scope="module")
def both(oracle_mod):
    if oracle_mod.reference_lib() is None:
        pytest.skip("neither oracle/_ref/libshs_ref_lib.so nor the reference tree to build it from is present")
    return oracle_mod


def _same_words(a, b, what):
    assert a.shape == b.shape and a.dtype == b.dtype, what
    w = a.view(np.uint32) if a.dtype == np.float32 else a
    v = b.view(np.uint32) if b.dtype == np.float32 else b
    bad = np.argwhere(w != v)
    assert bad.size == 0, f"{what}: {len(bad)} words differ, first at {bad[:3].tolist()}: oracle={a[tuple(bad[0])]!r} reference={b[tuple(bad[0])]!r}"
    _WORDS["words"] += int(w.size)


def _equal(o, frame, draws, sm=None):
    """oracle.pbr_forward == oracle.ref_pbr_forward in every word -> (hdr, depth, stats, covered)."""
    oh, od, om, ost = o.pbr_forward(frame, draws, sm)
    rh, rd, rm, rst = o.ref_pbr_forward(frame, draws, sm)
    assert ost == rst, (ost, rst)
    _same_words(oh, rh, "hdr")
    if frame.depth_motion:
        _same_words(od, rd, "depth")
        _same_words(om, rm, "motion")
        covered = int((rd < 1.0).sum())
    else:
        assert rd is None and od is None
        bg = np.asarray(frame.clear_hdr, np.float32)
        covered = int((rh != bg).any(axis=2).sum())
    assert rst["tri_after_clip"] > 0, rst
    if min(frame.width, frame.height) > 1:
        assert covered > 0 and rst["tri_raster"] > 0, (covered, rst)
    else:
        # a frame one pixel wide or high scales that screen axis by (W - 1) = 0: every triangle has zero area
        # and the reference rasterises none (rasterizer.hpp:267-274), which both sides must agree on
        assert covered == 0 and rst["tri_raster"] == 0, (covered, rst)
    _WORDS["cases"] += 1
    _WORDS["words"] += 3
    return rh, rd, rst, covered


def _shadowed(o, frame, draws, sm, depth):
    """Covered pixels whose colour the shadow term changes (at full strength), on the reference."""
    full, off = copy.deepcopy(draws), copy.deepcopy(draws)
    for d in full:
        d.shadow_strength = 1.0
    for d in off:
        d.shadow = False
    h1 = o.ref_pbr_forward(frame, full, sm)[0]
    h0 = o.ref_pbr_forward(frame, off, sm)[0]
    return int(((h1 != h0).any(axis=2) & (depth < 1.0)).sum())


# ---- the inputs of tests/test_lib_parity.py ----------------------------------------------------------

@pytest.mark.parametrize("pcf", [0, 1, 2])
@pytest.mark.parametrize("program", [0, 1, 2, 3, 4])
def test_c5_programs_and_pcf(both, program, pcf):
    from shs_gpu import scene_lib
    frame, draws, casters, sun, _ = scene_lib.c5_scene(160, 96, program=program)
    sm, lvp = both.shadow_map(64, sun, casters)
    scene_lib.wire_shadow(draws, lvp)
    for d in draws:
        d.shadow_pcf_radius = pcf
    _, rd, _, covered = _equal(both, frame, draws, sm)
    if program in (0, 1):
        assert 0 < _shadowed(both, frame, draws, sm, rd) < covered


def test_c5_shadow_map_sizes(both):
    """The two configurations of test_lib_parity.py::test_c5_shadow_map_sizes."""
    from shs_gpu import scene_lib
    frame, draws, casters, sun, _ = scene_lib.c5_scene(320, 200, yaw=-40.0)
    for size, radius, step in (((300, 170), 1, 1.0), (128, 0, 2.0)):
        sm, lvp = both.shadow_map(size, sun, casters)
        scene_lib.wire_shadow(draws, lvp)
        for d in draws:
            d.shadow_pcf_radius, d.shadow_pcf_step = radius, step
        _, rd, _, covered = _equal(both, frame, draws, sm)
        assert 0 < _shadowed(both, frame, draws, sm, rd) < covered


@pytest.mark.parametrize("W,H", [(1, 1), (1, 29), (37, 1), (16, 4), (65, 33)])
def test_tiny_frames(both, W, H):
    from shs_gpu import scene_lib
    frame, draws, casters, sun, _ = scene_lib.c5_scene(W, H, program=(W + H) % 5)
    sm, lvp = both.shadow_map(64, sun, casters)
    scene_lib.wire_shadow(draws, lvp)
    _equal(both, frame, draws, sm)


@pytest.mark.parametrize("seed", [1, 2])
@pytest.mark.parametrize("cull", [0, 1, 2])
def test_clip_soup(both, seed, cull):
    """test_lib_parity.py::test_clip_soup_exact's soup, camera and draw (motion vectors on)."""
    from shs_gpu.lib_path import LibDraw, LibFrame, LibMesh, model_euler
    rng = np.random.default_rng(seed)
    W, H = 331, 227
    pos, nrm, uv = _clip_soup(rng, 1200)
    mesh = LibMesh(pos, nrm[: len(nrm) - 7], uv)          # short normal array -> (0,1,0) defaults
    d = LibDraw(mesh=mesh, program=seed % 2, viewproj=_camera(W, H),
                model=model_euler((0.1, -0.2, 0.3), (0.2, 0.4, -0.1), (1.0, 1.2, 0.9)),
                prev_model=model_euler((0.0, -0.2, 0.3), (0.2, 0.45, -0.1), (1.0, 1.2, 0.9)), camera_pos=(0.3, 0.7, -3.0),
                cull_mode=cull, front_face_ccw=bool(seed % 2), enable_motion_vectors=True, light_intensity=3.0)
    frame = LibFrame(W, H, zn=0.5, zf=30.0)
    _, _, st, _ = _equal(both, frame, [d])
    # clipping happened: with culling off, more fan triangles come out than input triangles lie wholly inside
    # the frustum, so clipped polygons contributed theirs (the inside count in float64, a margin of hundreds)
    none = copy.copy(d)
    none.cull_mode = 0
    st0 = both.ref_pbr_forward(frame, [none])[3]
    M = (np.asarray(d.viewproj, np.float64).reshape(4, 4).T @ np.asarray(d.model, np.float64).reshape(4, 4).T)
    c = np.c_[pos.astype(np.float64), np.ones(len(pos))] @ M.T
    inside = ((c[:, 3:] > 0) & (np.abs(c[:, :3]) <= c[:, 3:])).all(axis=1).reshape(-1, 3).all(axis=1)
    assert st0["tri_after_clip"] > int(inside.sum()) + 100, (st0, int(inside.sum()))
    assert st["tri_after_clip"] > st["tri_raster"] // 2


def test_painter_mode_without_depth_target(both):
    from shs_gpu.lib_path import LibDraw, LibFrame, LibMesh
    rng = np.random.default_rng(5)
    W, H = 200, 150
    pos, nrm, uv = _clip_soup(rng, 600)
    vp = _camera(W, H)
    draws = [LibDraw(mesh=LibMesh(pos[:900], nrm[:900], uv[:900]), program=3, viewproj=vp, cull_mode=0),
             LibDraw(mesh=LibMesh(pos[900:], nrm[900:], uv[900:]), program=2, viewproj=vp, cull_mode=0,
                     base_color=(0.2, 0.9, 0.1))]
    _equal(both, LibFrame(W, H, depth_motion=False, bg_gradient=False, clear_hdr=(0.1, 0.2, 0.3, 1.0)), draws)


def test_linear_depth_off(both):
    """zf <= zn + 1e-6: the NDC depth is kept."""
    from shs_gpu.lib_path import LibDraw, LibFrame, LibMesh
    rng = np.random.default_rng(9)
    pos, nrm, uv = _clip_soup(rng, 500)
    _equal(both, LibFrame(160, 120, zn=1.0, zf=1.0), [LibDraw(mesh=LibMesh(pos, nrm, uv), viewproj=_camera(160, 120), cull_mode=0)])


def test_indexed_multi_draw(both):
    """test_lib_parity.py::test_indexed_grid_bins_mode's frame (16 indexed monkeys + C5, 2 programs, 3 cull modes)
    at half its size."""
    from shs_gpu import scene_lib
    from shs_gpu.lib_path import LibDraw, model_euler
    frame, draws, _, _, _ = scene_lib.c5_scene(256, 144)
    base = draws[1]
    for i in range(16):
        m = model_euler(((i % 4) * 3.0 - 4.5, 1.0 + (i // 4) * 0.4, (i // 4) * 3.0 - 2.0), (0.0, 0.3 * i, 0.0), (1.0, 1.0, 1.0))
        draws.append(LibDraw(mesh=base.mesh, program=i % 2, model=m, viewproj=base.viewproj,
                             prev_viewproj=base.prev_viewproj, light_dir_ws=base.light_dir_ws, light_intensity=5.0,
                             camera_pos=base.camera_pos, base_color=(0.2 + 0.05 * i, 0.5, 0.7), roughness=0.3,
                             cull_mode=i % 3, enable_motion_vectors=True))
    _, _, st, _ = _equal(both, frame, draws)
    assert st["tri_input"] > 4096


def test_reference_rejects_other_programs(both):
    from shs_gpu import scene_lib
    frame, draws, _, _, _ = scene_lib.c5_scene(16, 8, program=5)
    with pytest.raises(RuntimeError):
        both.ref_pbr_forward(frame, draws)


# ---- the uniform sweep -----------------------------------------------------------------------------

def _render_row(o, row):
    frame, draws, shadow = cases.sweep_scene(row)
    sm = None
    if shadow is not None:
        sm, lvp = o.shadow_map(*shadow)
        if row["sm"] == "synthetic":
            sm = cases.synthetic_shadow_map()
        cases.wire(row, draws, lvp)
    return frame, draws, sm


@pytest.mark.parametrize("row", cases.SWEEP, ids=[r["name"] for r in cases.SWEEP])
def test_sweep(both, row):
    frame, draws, sm = _render_row(both, row)
    rh, rd, _, covered = _equal(both, frame, draws, sm)
    assert np.isfinite(rh).all(), "the reference itself yields a finite colour for every row"
    if row["gpu"]:
        assert float(np.abs(rh).max()) < cases.GPU_HDR_CAP
    if cases.about_shadow(row):
        assert 0 < _shadowed(both, frame, draws, sm, rd) < covered


def test_sweep_covers_what_it_claims():
    """The table reaches every edge the sweep is about (so a later edit cannot quietly drop one)."""
    rows, g = cases.SWEEP, cases.SWEEP_GPU
    for p in (0, 1):
        mine = [r for r in g if r["program"] == p]
        assert any(r["ldir"] == "zero" for r in mine)
        assert any(r["roughness"] is not None and r["roughness"] < 0.04 for r in mine)
        assert any(r["roughness"] is not None and r["roughness"] > 1.0 for r in mine)
        assert any(r["metallic"] is not None and r["metallic"] < 0.0 for r in mine)
        assert any(r["metallic"] is not None and r["metallic"] > 1.0 for r in mine)
        assert any(r["base"] is not None and min(r["base"]) < 0.0 for r in mine)
        assert any(min(r["lcol"]) < 0.0 for r in mine)
    assert {(r["pcf_r"], r["pcf_step"]) for r in g} >= {(-1, 1.5), (-1, 2.5), (3, 1.5), (3, 2.5)}
    assert any(r["strength"] < 0.0 for r in g) and any(r["strength"] > 1.0 for r in g)
    assert any(r["sm"] == (1, 1) for r in g)
    assert any(r["tex"] == (1, 1) for r in g) and any(r["tex"] == (1, 7) for r in g)
    assert {r["pcf_r"] for r in rows} >= {-1, 0, 1, 2, 3} and {r["pcf_step"] for r in rows} >= {0.4, 1.0, 1.5, 2.5, 3.0}
    assert {r["inten"] for r in rows} >= {0.0, 1.0, 5.0}
    assert {r["tex"] for r in rows} >= {(1, 1), (1, 7), (6, 1), (5, 4)}
    assert {r["lvp"] for r in rows} == {"true", "outside", "border"}


# ---- PassTonemap / PassMotionBlur --------------------------------------------------------------------

@pytest.mark.parametrize("gamma", cases.TONEMAP_GAMMAS)
@pytest.mark.parametrize("exposure", [1.0, 2.5, 0.0])
def test_tonemap_synthetic(both, exposure, gamma):
    hdr = cases.synthetic_hdr()
    want = both.ref_tonemap(hdr, exposure, gamma)
    got, present = both.tonemap(hdr, exposure, gamma)
    _same_words(got, want, "ldr")
    assert np.array_equal(present, want[::-1])
    if gamma == 2.2 and exposure == 1.0:     # the boundaries were placed for this curve
        assert len(np.unique(want[..., :3])) == 256, "every byte value is reached"
    _WORDS["cases"] += 1


_MB_INPUTS = {}


def _mb_inputs(o, W, H):
    """One C5 frame of the reference through the reference's tonemap -> read-only (ldr, depth, motion)."""
    if (W, H) not in _MB_INPUTS:
        from shs_gpu import scene_lib
        frame, draws, _, _, _ = scene_lib.c5_scene(W, H)
        hdr, depth, motion, _ = o.ref_pbr_forward(frame, draws)
        ldr = o.ref_tonemap(hdr, 1.0, 2.2)
        for a in (ldr, depth, motion):
            a.setflags(write=False)
        _MB_INPUTS[(W, H)] = (ldr, depth, motion)
    return _MB_INPUTS[(W, H)]


@pytest.mark.parametrize("case", range(len(MB_CASES)))
def test_motion_blur_cases(both, case):
    params = MB_CASES[case]
    ldr, depth, motion = _mb_inputs(both, 352, 200)      # test_post.py::test_motion_blur_exact's frame
    assert np.abs(motion).max() > 1.0, "scene has no motion to blur"
    want = both.ref_motion_blur(ldr, depth, motion, **params)
    _same_words(both.motion_blur(ldr, depth, motion, **params), want, "motion blur")
    if params.get("enable", True) and params.get("strength", 1.0) > 0:
        assert not np.array_equal(want, ldr), "blur changed nothing"
    else:
        assert np.array_equal(want, ldr)
    _WORDS["cases"] += 1


def test_motion_blur_nonfinite_motion(both):
    ldr, depth, _ = _mb_inputs(both, 160, 96)
    mot = cases.nonfinite_motion(160, 96)
    assert np.isnan(mot).any() and np.isinf(mot).any()
    want = both.ref_motion_blur(ldr, depth, mot, min_velocity_px=0.0)
    _same_words(both.motion_blur(ldr, depth, mot, min_velocity_px=0.0), want, "motion blur (non-finite motion)")
    assert not np.array_equal(want, ldr)
    _WORDS["cases"] += 1


def test_zz_tally(both):
    print(f"\noracle == compiled reference: {_WORDS['cases']} cases, {_WORDS['words']} words and bytes compared, 0 differences")
    assert _WORDS["cases"] > 0
