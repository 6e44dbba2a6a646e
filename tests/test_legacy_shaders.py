"""The Toon, Gooch, Oren-Nayar, normal- and depth-visualiser shading models of the legacy raster on the GPU
against tests/legacy_shaders_ref (test_legacy_shaders_ref.py holds the wrapper, the scenes and what pins the
reference on the CPU).

Depth is bit-exact and coverage equal everywhere.  The visualisers' bytes equal the reference's; Gooch, Toon
and Oren-Nayar pass helpers.assert_color_parity as it stands, Toon without the pixels whose specular power is
within TOL of its 0.5 step, Oren-Nayar without those with cos(beta) < 2^-7 (where tan(beta) turns one ulp of
acosf into more than TOL) -- never more than 0.5 % of a frame's covered pixels.

Frames: one per model in scan and bin mode; nine overlapping draws, one per model 0..8, with tile groups on
and off; batches of single-draw and two-draw frames; shared varyings; two shards; a one-device group.
Samples (legacy_shade_samples): the Toon thresholds either side, the specular step, Oren-Nayar's NaN path and
exact zeros, the depth visualiser's clamps and NaN, a zero normal sum, and the rejections."""
import copy

import numpy as np
import pytest

import helpers
from test_legacy_shaders_ref import (BLINN, CAP, COLOR, DEPTH_VIS, F, GOOCH, H, NEW_MODELS, NORMAL_VIS, OREN, POSES, TOON, W,
                                     covered, edge_sets, excusable, frame_desc, mixed_frame, model_frame, monkey_draw,
                                     random_varyings, ref_render, ref_samples, same_bits, LIGHT, CAM)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctxs():
    """Contexts by raster variant: scan, bins, scan with a work item per tile (no tile groups)."""
    import shs_gpu
    cs = {k: shs_gpu.Context(0) for k in ("scan", "bins", "tiles")}
    cs["scan"].set_raster_mode(1)
    cs["bins"].set_raster_mode(2)
    cs["tiles"].set_raster_mode(1)
    cs["tiles"].set_tile_groups(False)
    yield cs
    for c in cs.values():
        c.close()


def _planes(ctx, k=0):
    color, depth = ctx.resolve_frame(k)
    return {"color": color, "depth": depth, "prequant": ctx.resolve_prequant(k)}


def _check_against_reference(got, ref, mask_of_model):
    """got / ref: plane dicts.  mask_of_model: model -> the canvas-row mask of the pixels that model shades
    (the reference judges these; the others are someone else's).  Returns the excused pixel count."""
    helpers.assert_depth_bitexact(got["depth"], ref["depth"])
    assert np.array_equal(got["color"][..., 3], ref["color"][..., 3])
    excused = 0
    for m, mine in mask_of_model.items():
        skip = excusable(m, ref) & mine
        n_mine = int(mine.sum())
        assert int(skip.sum()) <= CAP * n_mine, f"model {m}: {int(skip.sum())} of {n_mine} pixels excused"
        excused += int(skip.sum())
        judge = mine & ~skip
        g_c, r_c = np.where(judge[..., None], got["color"], 0), np.where(judge[..., None], ref["color"], 0)
        if m in (NORMAL_VIS, DEPTH_VIS):
            assert np.array_equal(g_c, r_c), f"model {m}: colour bytes differ"
            assert same_bits(got["prequant"][judge], ref["prequant"][judge]).all(), f"model {m}: floats differ"
        else:
            g_p, r_p = np.where(judge[..., None], got["prequant"], 0), np.where(judge[..., None], ref["prequant"], 0)
            helpers.assert_color_parity(g_c, r_c, g_p, r_p)
            d = np.abs(g_p[..., :3] - r_p[..., :3])
            assert d.max() <= helpers.TOL * 255.0, f"model {m}: pre-truncation floats differ by {d.max()}"
    return excused


@pytest.mark.parametrize("mode", ["scan", "bins"])
@pytest.mark.parametrize("model", NEW_MODELS)
def test_one_frame_per_model(ctxs, model, mode):
    draws, ref = model_frame(model)
    c = ctxs[mode]
    c.render(frame_desc(), draws)
    got = _planes(c)
    n = int(covered(ref).sum())
    assert c.stats()["covered_pixels"] == n
    _check_against_reference(got, ref, {model: covered(ref)})


@pytest.mark.parametrize("variant", ["scan", "tiles", "bins"])
def test_mixed_frame_of_all_nine_models(ctxs, oracle_mod, variant):
    """Two frames of the nine draws (a batch, so that the scan context runs tile groups): the new models'
    pixels against the reference, the Flat .. Blinn-Phong pixels against the oracle."""
    draws, ref = mixed_frame()
    sub = [copy.copy(d) for d in draws]
    for d in sub[4:]:
        d.shading = BLINN
    ora_c, ora_d, ora_pq = oracle_mod.render_legacy(W, H, sub, prequant=True)
    c = ctxs[variant]
    c.render_batch(frame_desc(), [draws, draws])
    for k in range(2):
        got = _planes(c, k)
        _check_against_reference(got, ref, {m: ref["draw_id"] == m for m in NEW_MODELS})
        old = (ref["draw_id"] >= 0) & (ref["draw_id"] <= BLINN)
        assert old.sum() > 300
        helpers.assert_depth_bitexact(got["depth"], ora_d)
        helpers.assert_color_parity(np.where(old[..., None], got["color"], 0), np.where(old[..., None], ora_c, 0),
                                    np.where(old[..., None], got["prequant"], 0), np.where(old[..., None], ora_pq, 0))


@pytest.mark.parametrize("variant", ["scan", "tiles", "bins"])
def test_frame_of_the_four_old_models_alone(ctxs, oracle_mod, variant):
    """The path of a batch without a new model is intact: the mixed frame's first four draws against the oracle."""
    draws = mixed_frame()[0][:4]
    ora_c, ora_d, ora_pq = oracle_mod.render_legacy(W, H, draws, prequant=True)
    c = ctxs[variant]
    c.render_batch(frame_desc(), [draws, draws])
    for k in range(2):
        got = _planes(c, k)
        helpers.assert_depth_bitexact(got["depth"], ora_d)
        helpers.assert_color_parity(got["color"], ora_c, got["prequant"], ora_pq)


def _single(ctx, draws, **kw):
    ctx.render(frame_desc(**kw), draws)
    return _planes(ctx)


def _same_planes(a, b):
    assert np.array_equal(a["depth"].view(np.uint32), b["depth"].view(np.uint32))
    assert np.array_equal(a["color"], b["color"])
    assert same_bits(a["prequant"], b["prequant"]).all()


@pytest.mark.parametrize("two_draws", [False, True])
def test_batch_frames_equal_their_single_frames(ctxs, two_draws):
    """Five frames, one new model and camera pose each, in one batch with tile groups on: the single-draw
    frames take the group resolve's scalar branch, the two-draw frames its fallback."""
    fds = []
    for k, m in enumerate(NEW_MODELS):
        d = [monkey_draw(m, **POSES[k])]
        if two_draws:
            d.append(monkey_draw(NEW_MODELS[(k + 2) % 5], position=(2.0, 1.0, 13.0), scale=3.0, **POSES[k]))
        fds.append(d)
    c = ctxs["scan"]
    c.render_batch(frame_desc(), fds)
    got = [_planes(c, k) for k in range(5)]
    for k in range(5):
        _same_planes(got[k], _single(ctxs["tiles"], fds[k]))
    if not two_draws:   # and the reference itself, under each pose
        for k, m in enumerate(NEW_MODELS):
            ref = ref_render(W, H, fds[k])
            _check_against_reference(got[k], ref, {m: covered(ref)})


@pytest.mark.parametrize("model", [TOON, DEPTH_VIS])
def test_batch_of_poses_with_one_model_matrix(ctxs, model):
    """Three poses of one model matrix: Toon's varyings are shared by the batch, the depth visualiser's (the
    clip z, which the pose changes) must not be; either way each frame is its single-frame render."""
    fds = [[monkey_draw(model, **POSES[k])] for k in range(3)]
    for name in ("scan", "bins"):
        c = ctxs[name]
        c.render_batch(frame_desc(), fds)
        got = [_planes(c, k) for k in range(3)]
        for k in range(3):
            _same_planes(got[k], _single(ctxs["tiles"], fds[k]))
    ref = ref_render(W, H, fds[2])
    _check_against_reference(got[2], ref, {model: covered(ref)})


def test_two_shards_make_the_unsharded_frame(ctxs):
    draws = mixed_frame()[0]
    want = _single(ctxs["scan"], draws)
    T = 32                          # shs_gpu_tile_size(): rank r owns the 32x32 tiles t with t % 2 == r, row-major
    tx, ty = (W + T - 1) // T, (H + T - 1) // T
    color = np.zeros_like(want["color"])
    depth = np.zeros_like(want["depth"])
    pq = np.zeros_like(want["prequant"])
    for r in range(2):
        part = _single(ctxs["scan"], draws, shard_rank=r, shard_count=2)
        for t in range(r, tx * ty, 2):
            x0, y0 = (t % tx) * T, (t // tx) * T
            x1, y1 = min(x0 + T, W), min(y0 + T, H)
            depth[y0:y1, x0:x1] = part["depth"][y0:y1, x0:x1]
            color[H - y1:H - y0, x0:x1] = part["color"][H - y1:H - y0, x0:x1]
            pq[H - y1:H - y0, x0:x1] = part["prequant"][H - y1:H - y0, x0:x1]
    _same_planes({"color": color, "depth": depth, "prequant": pq}, want)


def test_group_legacy_call_with_oren_nayar(ctxs):
    from shs_gpu.group import Group
    draws = model_frame(OREN)[0]
    frame = frame_desc(present=True)
    single = ctxs["scan"]
    single.render(frame, draws)
    want = single.resolve_present(0)
    g = Group([0])
    try:
        g.render(frame, draws)
        g.gather(single.TARGET_PRESENT)
        assert np.array_equal(g.root.resolve_present(0), want)
    finally:
        g.close()
    assert (want[..., :3] != 0).any()


# ---- samples ------------------------------------------------------------------------------------------------
def _check_samples(ctx, model, light, cam, ns, wp, cz):
    ref = ref_samples(model, light, cam, COLOR, ns, wp, cz)
    rgba, pq = ctx.legacy_shade_samples(model, light, cam, COLOR, ns, wp, cz)
    keep = ~excusable(model, ref)
    assert np.array_equal(rgba[:, 3], ref["rgba"][:, 3]) and (pq[:, 3] == 1.0).all()
    assert np.array_equal(np.isnan(pq), np.isnan(ref["prequant"]))
    if model in (NORMAL_VIS, DEPTH_VIS):
        assert np.array_equal(rgba, ref["rgba"])
        assert same_bits(pq, ref["prequant"]).all()
        return ref, rgba, keep
    d = np.abs(pq[keep, :3].astype(np.float64) - ref["prequant"][keep, :3])
    d = d[~np.isnan(d)]
    assert d.size == 0 or d.max() <= helpers.TOL * 255.0, d.max()
    # a byte off by one only on a truncation boundary the floats straddle within TOL (assert_color_parity's rule)
    d8 = np.abs(rgba[keep].astype(np.int16) - ref["rgba"][keep].astype(np.int16))
    assert d8.max(initial=0) <= 1
    return ref, rgba, keep


@pytest.mark.parametrize("model", NEW_MODELS)
def test_samples_random_varyings(ctxs, model):
    ns, wp, cz = random_varyings(600, 11 + model)
    ref, rgba, keep = _check_samples(ctxs["scan"], model, np.asarray(LIGHT, F), CAM, ns, wp, cz)
    # (Oren-Nayar: a random normal faces away from light and viewer about one time in three -- cos(beta) = 0)
    assert keep.sum() >= (0.4 if model == OREN else 0.98) * keep.size


def test_samples_toon_thresholds_and_specular(ctxs):
    sets = edge_sets()[TOON]
    light, cam, ns, wp, cz = sets[0]           # the five thresholds, the two floats either side of each
    ref = ref_samples(TOON, light, cam, COLOR, ns, wp, cz)
    rgba, pq = ctxs["scan"].legacy_shade_samples(TOON, light, cam, COLOR, ns, wp, cz)
    assert (ref["spec_margin"] > helpers.TOL).all()
    assert np.array_equal(rgba, ref["rgba"]), "a band or rim decision differs from the reference's"
    assert same_bits(pq, ref["prequant"]).all()   # no pow in what differs: the same floats
    light, cam, ns, wp, cz = sets[1]           # the specular step, both sides
    ref, rgba, keep = _check_samples(ctxs["scan"], TOON, light, cam, ns, wp, cz)
    assert np.array_equal(rgba[keep], ref["rgba"][keep])
    on = ref["rgba"][:, 0] >= 204
    assert (keep & on).sum() > 10 and (keep & ~on).sum() > 10


def test_samples_oren_nayar_edges(ctxs):
    light, cam, ns, wp, cz = edge_sets()[OREN][0]
    ref = ref_samples(OREN, light, cam, COLOR, ns, wp, cz)
    rgba, pq = ctxs["scan"].legacy_shade_samples(OREN, light, cam, COLOR, ns, wp, cz)
    assert np.array_equal(rgba, ref["rgba"])
    assert rgba[0].tolist() == [0, 0, 0, 255] and np.isnan(pq[0, :3]).all()   # V parallel to N: NaN, byte 0
    assert np.array_equal(np.isnan(pq), np.isnan(ref["prequant"]))
    fin = ~np.isnan(ref["prequant"])
    assert np.abs(pq[fin] - ref["prequant"][fin]).max() <= helpers.TOL * 255.0


def test_samples_visualiser_edges(ctxs):
    for model in (DEPTH_VIS, NORMAL_VIS):
        light, cam, ns, wp, cz = edge_sets()[model][0]
        ref, rgba, _ = _check_samples(ctxs["scan"], model, light, cam, ns, wp, cz)
        if model == DEPTH_VIS:
            assert rgba[:, 0].tolist() == [255, 255, 0, 0, 0, 0, 167]
        else:
            assert rgba[0].tolist() == [0, 0, 0, 255]


def test_samples_blinn_phong_and_gooch_specular(ctxs):
    light, cam, ns, wp, cz = edge_sets()[GOOCH][0]
    _check_samples(ctxs["scan"], GOOCH, light, cam, ns, wp, cz)
    _check_samples(ctxs["scan"], BLINN, light, cam, ns, wp, cz)


def test_rejections(ctxs):
    import shs_gpu
    c = ctxs["scan"]
    one = np.ones((1, 3), F)
    for bad in (shs_gpu.SHADING_FLAT, shs_gpu.SHADING_GOURAUD, 9, -1):
        with pytest.raises(shs_gpu.ShsError, match="bad shading model"):
            c.legacy_shade_samples(bad, LIGHT, CAM, COLOR, one, one, [0.0])
    for bad in (9, -1):
        d = copy.copy(model_frame(TOON)[0][0])
        d.shading = bad
        with pytest.raises(shs_gpu.ShsError, match="bad shading model"):
            c.render(frame_desc(), [d])
