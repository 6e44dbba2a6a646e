"""The Canvas-API post passes on the GPU -- shs_canvas_velocity_blur, _fog, _outline, _fxaa, _spec_bright, _additive,
_lens_flare and the two frame entries -- against tests/canvas_fx_ref (test_canvas_fx_ref.py holds the wrapper, the
inputs, the parameter sets, the chains' restatement and what pins the reference on the CPU).

  * velocity blur, outline, FXAA, bright pass, additive: exact float arithmetic, so byte for byte the restatement's;
  * fog and flare hold the one transcendental each (pow, exp), a double evaluation rounded once on the device and the
    float libm in the restatement: the bytes go through helpers.assert_color_parity with the prequant planes, every
    byte off by one explained by its float.  The count is printed and not capped.  The floats themselves stay within
    helpers.TOL * 255 (one ulp of a factor in [0, 1] on a value of a few hundred is under 1e-4);
  * a pixel the fog only copies keeps its four bytes and has (0, 0, 0, -1) in the prequant plane;
  * a frame entry equals, bit for bit, the single-pass entries called in the demo's order; and along that order every
    step equals the restatement's step on the same input under the rules above -- a fog or flare byte off by one would
    otherwise make the later exact steps incomparable.  Whether the restatement's own chain ends in the same bytes is
    printed."""
import ctypes

import numpy as np
import pytest

import helpers
import test_canvas_fx_ref as R
import test_canvas_rt_ref as RT
from test_canvas_fx_ref import F, SIZES, SWEEP

pytestmark = pytest.mark.gpu
COPIED = np.array([0, 0, 0, -1], F)
_ids = lambda s: f"{s[0]}x{s[1]}"


@pytest.fixture(scope="module")
def ctx():
    import shs_gpu
    c = shs_gpu.Context(0)
    yield c
    c.close()


def _check_pq(got_c, got_pq, ref, label, src=None):
    """fog (src given: the copied-pixel rule) or flare against the restatement's dict(color, pq, branch)."""
    if src is not None:
        copied = ref["branch"] == 0
        assert np.array_equal(got_c[copied], src[copied]), f"{label}: a copied pixel changed"
        assert np.array_equal(got_pq[copied], np.broadcast_to(COPIED, got_pq[copied].shape)), f"{label}: a copied pixel's prequant"
        assert (got_pq[..., 3][~copied] == 1).all(), f"{label}: a fogged pixel was copied"
    else:
        assert (got_pq[..., 3] == 1).all()
    n = helpers.assert_color_parity(got_c, ref["color"], got_pq, ref["pq"])
    err = np.abs(got_pq[..., :3].astype(np.float64) - ref["pq"][..., :3].astype(np.float64))
    print(f"{label}: {n} bytes off by one, largest pre-conversion float difference {err.max():.3g} (bar {helpers.TOL * 255:.3g})")
    assert err.max() <= helpers.TOL * 255.0, f"{label}: pre-conversion floats differ by {err.max()}"


# ---- every pass at every size ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("size", SIZES, ids=_ids)
def test_exact_passes_equal_the_restatement(ctx, size):
    inp = R.inputs(size)
    src, depth, vel, spec = inp["src"], inp["depth"], inp["vel"], inp["spec"]
    assert np.array_equal(ctx.canvas_velocity_blur(src, vel), R.ref_velocity_blur(src, vel))
    assert np.array_equal(ctx.canvas_outline(src, depth), R.ref_outline(src, depth))
    assert np.array_equal(ctx.canvas_fxaa(src), R.ref_fxaa(src))
    bright = ctx.canvas_spec_bright(spec)
    assert np.array_equal(bright, R.ref_spec_bright(spec))
    assert np.array_equal(ctx.canvas_additive(src, bright), R.ref_additive(src, bright))


@pytest.mark.parametrize("size", SIZES, ids=_ids)
def test_fog_and_flare_equal_the_restatement(ctx, size):
    inp = R.inputs(size)
    got_c, got_pq = ctx.canvas_fog(inp["src"], inp["depth"], prequant=True)
    _check_pq(got_c, got_pq, R.fog_case("demo", size), f"fog {size}", inp["src"])
    got_c, got_pq = ctx.canvas_lens_flare(R.bloom_input(size), prequant=True)
    _check_pq(got_c, got_pq, R.flare_case("demo", size), f"flare {size}")
    assert np.array_equal(ctx.canvas_lens_flare(R.bloom_input(size)), got_c)      # the same bytes without the plane


# ---- parameter sweeps at 67 x 45 -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("radius", [0, 1, 2, 4])
def test_outline_radius(ctx, radius):
    from shs_gpu import _abi
    assert _abi.CANVAS_MAX_OUTLINE_RADIUS == 4
    inp = R.inputs(SWEEP)
    for thr, strength in ((0.75, 0.15), (0.1, 1.0), (5.0, 1.7)):
        want, br = R.ref_outline(inp["src"], inp["depth"], branch=True, radius=radius, threshold=thr, strength=strength)
        assert np.array_equal(ctx.canvas_outline(inp["src"], inp["depth"], radius=radius, threshold=thr, strength=strength), want)
        assert (radius == 0) == (R.OUTLINE_EDGE not in br)


@pytest.mark.parametrize("samples", [1, 2, 12, 32])
def test_velocity_blur_samples(ctx, samples):
    inp = R.inputs(SWEEP)
    for strength in (1.0, 1.5, 40.0):        # 40: taps far outside the canvas, clamped
        want = R.ref_velocity_blur(inp["src"], inp["vel"], samples=samples, strength=strength)
        assert np.array_equal(ctx.canvas_velocity_blur(inp["src"], inp["vel"], samples=samples, strength=strength), want)


@pytest.mark.parametrize("name", list(R.FOG_SETS))
def test_fog_parameter_sets(ctx, name):
    inp = R.inputs(SWEEP)
    got_c, got_pq = ctx.canvas_fog(inp["src"], inp["depth"], prequant=True, **R.FOG_SETS[name])
    _check_pq(got_c, got_pq, R.fog_case(name, SWEEP), f"fog {name}", inp["src"])


@pytest.mark.parametrize("name", list(R.FLARE_SETS))
def test_flare_parameter_sets(ctx, name):
    assert [len(R.FLARE_SETS[n].get("ghost_scales", (0,) * 3)) for n in ("one_ghost", "demo", "eight_ghosts")] == [1, 3, 8]
    got_c, got_pq = ctx.canvas_lens_flare(R.bloom_input(SWEEP), prequant=True, **R.FLARE_SETS[name])
    _check_pq(got_c, got_pq, R.flare_case(name, SWEEP), f"flare {name}")


def test_bright_threshold_one_and_additive_strengths(ctx):
    inp = R.inputs(SWEEP)
    spec = inp["spec"]
    for thr, inten in ((1.0, 1.0), (1.0, 13.25), (0.0, 0.5), (0.139, -2.0)):
        assert np.array_equal(ctx.canvas_spec_bright(spec, threshold=thr, intensity=inten),
                              R.ref_spec_bright(spec, threshold=thr, intensity=inten)), (thr, inten)
    assert (R.ref_spec_bright(spec, threshold=1.0, intensity=1.0)[..., :3] > 0).any()      # the 1e-6 floor lets > 1 through
    add = R.bloom_input(SWEEP)
    for k in (0.0, 1.0, 1.75, 300.0, -1.0):
        assert np.array_equal(ctx.canvas_additive(inp["src"], add, k), R.ref_additive(inp["src"], add, k)), k
    assert not np.array_equal(R.ref_additive(inp["src"], add, 1.75), R.ref_additive(inp["src"], add, 1.0))


# ---- device pointers -------------------------------------------------------------------------------------------------------

def test_device_tensors_equal_host_buffers(ctx):
    import torch
    size = (65, 5)
    inp = R.inputs(size)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a).copy()).cuda()
    src, depth, vel, spec, bloom = t(inp["src"]), t(inp["depth"]), t(inp["vel"]), t(inp["spec"]), t(R.bloom_input(size))
    host = lambda a: a.cpu().numpy()
    pairs = [
        (ctx.canvas_velocity_blur(src, vel), ctx.canvas_velocity_blur(inp["src"], inp["vel"])),
        (ctx.canvas_outline(src, depth), ctx.canvas_outline(inp["src"], inp["depth"])),
        (ctx.canvas_fxaa(src), ctx.canvas_fxaa(inp["src"])),
        (ctx.canvas_spec_bright(spec), ctx.canvas_spec_bright(inp["spec"])),
        (ctx.canvas_additive(src, bloom, 0.7), ctx.canvas_additive(inp["src"], R.bloom_input(size), 0.7)),
    ]
    ctx.synchronize()
    for k, (dev, hst) in enumerate(pairs):
        assert np.array_equal(host(dev), hst), k
    for dev, hst in ((ctx.canvas_fog(src, depth, prequant=True), ctx.canvas_fog(inp["src"], inp["depth"], prequant=True)),
                     (ctx.canvas_lens_flare(bloom, prequant=True), ctx.canvas_lens_flare(R.bloom_input(size), prequant=True))):
        ctx.synchronize()
        assert np.array_equal(host(dev[0]), hst[0]) and np.array_equal(host(dev[1]).view(np.uint32), hst[1].view(np.uint32))
    # in place: the additive pass onto its base (hello_glowing_star.cpp:1310), the fog onto its source
    base = src.clone()
    assert ctx.canvas_additive(base, bloom, 1.0, out=base) is base
    fogged = src.clone()
    assert ctx.canvas_fog(fogged, depth, dst=fogged) is fogged
    ctx.synchronize()
    assert np.array_equal(host(base), R.ref_additive(inp["src"], R.bloom_input(size), 1.0))
    assert np.array_equal(host(fogged), ctx.canvas_fog(inp["src"], inp["depth"]))
    with pytest.raises(ValueError):
        ctx.canvas_outline(src, inp["depth"])


# ---- the frame entries -----------------------------------------------------------------------------------------------------

def _gpu_step(ctx, step, cur, inp, params):
    p = params.get(step) or {}
    if step == "velocity_blur":
        return ctx.canvas_velocity_blur(cur, inp["vel"], **p), None
    if step == "motion_blur":
        return ctx.canvas_motion_blur(cur, inp["depth"], inp["vel"], **p), None
    if step == "dof":
        import shs_gpu
        q = dict(shs_gpu.Context.FX_DEFAULTS["dof"], **p)
        return ctx.canvas_dof(cur.copy(), inp["depth"], **q)[0], None
    if step == "fog":
        return ctx.canvas_fog(cur, inp["depth"], prequant=True, **p)
    if step == "outline":
        return ctx.canvas_outline(cur, inp["depth"], **p), None
    return ctx.canvas_fxaa(cur, **p), None


def _check_multi_pass(ctx, size, blur_mode, enable_dof, enable_fxaa, params):
    inp = R.inputs(size)
    label = f"multi-pass {size} mode {blur_mode} dof {enable_dof} fxaa {enable_fxaa}"
    cur = inp["src"]
    for step in R.multi_pass_steps(blur_mode, enable_dof, enable_fxaa):
        got, got_pq = _gpu_step(ctx, step, cur, inp, params)
        if step == "fog":
            _check_pq(got, got_pq, R.ref_fog(cur, inp["depth"], **(params.get("fog") or {})), f"{label}: fog", cur)
        else:
            assert np.array_equal(got, R.ref_step(step, cur, inp, params)[0]), f"{label}: {step}"
        cur = got
    frame = ctx.canvas_multi_pass_frame(inp["src"], inp["depth"], inp["vel"], blur_mode=blur_mode, enable_dof=enable_dof,
                                        enable_fxaa=enable_fxaa, **params)
    assert np.array_equal(frame, cur), f"{label}: the frame entry differs from its passes called one by one"
    pure = R.ref_multi_pass_frame(inp, blur_mode, enable_dof, enable_fxaa, **params)
    print(f"{label}: {int((frame != pure).sum())} bytes differ from the restatement's own chain")
    return frame


@pytest.mark.parametrize("flags", [(True, True), (False, True), (True, False), (False, False)], ids=lambda f: f"dof{int(f[0])}-fxaa{int(f[1])}")
@pytest.mark.parametrize("blur_mode", [0, 1, 2])
def test_multi_pass_frame(ctx, blur_mode, flags):
    params = dict(motion_blur=R.camera_pair(SWEEP)) if blur_mode else {}
    _check_multi_pass(ctx, SWEEP, blur_mode, flags[0], flags[1], params)


def test_multi_pass_frame_with_other_parameters(ctx):
    params = dict(velocity_blur=dict(samples=5, strength=2.0), dof=dict(iterations=1, radius=2, range_=10.0, max_blur=1.0),
                  fog=dict(fog_color=(200, 10, 90, 0), fog_start=10.0, fog_end=60.0, fog_power=0.5),
                  outline=dict(radius=2, threshold=3.0, strength=0.6), fxaa=dict(reduce_min=1.0 / 64.0, reduce_mul=0.25, span_max=4.0))
    a = _check_multi_pass(ctx, (128, 96), 0, True, True, params)
    b = _check_multi_pass(ctx, (128, 96), 0, True, True, {})
    assert not np.array_equal(a, b)


def _check_glow(ctx, size, enable_dof, enable_bloom, enable_flare, iters, params):
    import shs_gpu
    inp = R.inputs(size)
    label = f"glow {size} dof {enable_dof} bloom {enable_bloom} flare {enable_flare}"
    p = R.glow_params(params)
    black = np.zeros_like(inp["src"])
    black[..., 3] = 255
    mb = ctx.canvas_velocity_blur(inp["src"], inp["vel"], **p["velocity_blur"])
    assert np.array_equal(mb, R.ref_velocity_blur(inp["src"], inp["vel"], **p["velocity_blur"])), label
    dof = mb
    if enable_dof:
        dof = ctx.canvas_dof(mb.copy(), inp["depth"], **dict(shs_gpu.Context.FX_DEFAULTS["dof"], **p["dof"]))[0]
        assert np.array_equal(dof, R.ref_dof(mb, inp["depth"], **p["dof"])), label
    bloom = black
    if enable_bloom:
        bloom = ctx.canvas_spec_bright(inp["spec"], **p["spec_bright"])
        for _ in range(iters):
            bloom = ctx.canvas_gaussian_blur(ctx.canvas_gaussian_blur(bloom, True), False)
    flare = black
    if enable_flare:
        flare, flare_pq = ctx.canvas_lens_flare(bloom, prequant=True, **p["lens_flare"])
        _check_pq(flare, flare_pq, R.ref_lens_flare(bloom, **p["lens_flare"]), f"{label}: flare")
    final = ctx.canvas_additive(ctx.canvas_additive(dof, bloom), flare)
    assert np.array_equal(final, R.ref_additive(R.ref_additive(dof, bloom), flare)), label
    st = R.ref_glow_frame(inp, enable_dof, enable_bloom, enable_flare, iters, stages=True, **params)
    assert np.array_equal(bloom, st["bloom"]), f"{label}: bloom"
    frame = ctx.canvas_glow_frame(inp["src"], inp["depth"], inp["vel"], inp["spec"], enable_dof=enable_dof,
                                  enable_bloom=enable_bloom, enable_flare=enable_flare, bloom_iterations=iters, **params)
    assert np.array_equal(frame, final), f"{label}: the frame entry differs from its passes called one by one"
    print(f"{label}: {int((frame != st['final']).sum())} bytes differ from the restatement's own chain")
    return frame


@pytest.mark.parametrize("flags", [(1, 1, 1), (0, 1, 1), (1, 0, 1), (1, 1, 0), (0, 0, 0)], ids=lambda f: "dof%d-bloom%d-flare%d" % f)
def test_glow_frame(ctx, flags):
    frame = _check_glow(ctx, SWEEP, bool(flags[0]), bool(flags[1]), bool(flags[2]), 10, {})
    if flags == (0, 0, 0):       # black bloom and flare: the motion-blurred frame with alpha 255
        inp = R.inputs(SWEEP)
        mb = R.ref_velocity_blur(inp["src"], inp["vel"], samples=8, strength=1.5)
        assert np.array_equal(frame[..., :3], mb[..., :3]) and (frame[..., 3] == 255).all()


def test_glow_frame_without_iterations_and_with_other_parameters(ctx):
    _check_glow(ctx, (128, 96), True, True, True, 0, {})
    _check_glow(ctx, (128, 96), True, True, True, 3, dict(spec_bright=dict(threshold=0.3, intensity=4.0),
                                                         lens_flare=dict(ghost_scales=(0.4, 1.1), chroma_shift_px=2.5)))


def test_frames_on_device_tensors_and_scratch_regrowth(ctx):
    """Device tensors equal host buffers; on one context a larger then a smaller canvas (the scratch canvases regrow, then
    are larger than needed) and the first size again."""
    import torch
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a).copy()).cuda()
    first = None
    for size in ((65, 5), (128, 96), (64, 4), (65, 5)):
        inp = R.inputs(size)
        cam = R.camera_pair(size)
        host_m = ctx.canvas_multi_pass_frame(inp["src"], inp["depth"], inp["vel"], blur_mode=2, motion_blur=cam)
        host_g = ctx.canvas_glow_frame(inp["src"], inp["depth"], inp["vel"], inp["spec"], bloom_iterations=2)
        dev = [t(inp[k]) for k in ("src", "depth", "vel", "spec")]
        dev_m = ctx.canvas_multi_pass_frame(dev[0], dev[1], dev[2], blur_mode=2, motion_blur=cam)
        dev_g = ctx.canvas_glow_frame(*dev, bloom_iterations=2)
        color = dev[0].clone()
        assert ctx.canvas_multi_pass_frame(color, dev[1], dev[2], dst=color) is color      # dst may be color
        ctx.synchronize()
        assert np.array_equal(dev_m.cpu().numpy(), host_m) and np.array_equal(dev_g.cpu().numpy(), host_g), size
        assert np.array_equal(color.cpu().numpy(), ctx.canvas_multi_pass_frame(inp["src"], inp["depth"], inp["vel"])), size
        if first is None:
            first = (host_m, host_g)
    assert np.array_equal(host_m, first[0]) and np.array_equal(host_g, first[1])
    import shs_gpu
    with shs_gpu.Context(0) as fresh:
        inp = R.inputs((65, 5))
        assert np.array_equal(fresh.canvas_glow_frame(inp["src"], inp["depth"], inp["vel"], inp["spec"], bloom_iterations=2), first[1])


def test_frame_after_the_raster_on_the_device(ctx):
    """shs_rt_render -> shs_rt_device_targets -> shs_canvas_multi_pass_frame at the demos' 380 x 280, all on the device,
    against the same chain over the resolved host copies of the targets."""
    import torch
    w, h = 380, 280
    view, lvp, draws = RT.scene_demo()
    ctx._on_torch_stream()
    ctx.rt_render_shadow(RT.SM, lvp, draws)
    ctx.rt_render(RT._frame(view, lvp, w=w, h=h), draws)
    color, depth, vel = ctx.rt_resolve()
    assert (depth != helpers.FLT_MAX).sum() > 1000 and (depth == helpers.FLT_MAX).any() and np.abs(vel).max() > 0.5
    want = ctx.canvas_multi_pass_frame(color, depth, vel)
    ctx.rt_render(RT._frame(view, lvp, w=w, h=h), draws)
    c_dev, d_dev, v_dev = ctx.rt_device_targets()
    dst = torch.empty((h, w, 4), dtype=torch.uint8, device="cuda")
    d = ctx.multi_pass_frame_desc(w, h)
    _P = ctypes.c_void_p
    ctx._check(ctx._lib.shs_canvas_multi_pass_frame(ctx._h, ctypes.byref(d), _P(c_dev), _P(d_dev), _P(v_dev), _P(dst.data_ptr()),
                                                    ctx.CANVAS_DEVICE))
    ctx.synchronize()
    assert np.array_equal(dst.cpu().numpy(), want)
    assert np.array_equal(ctx.rt_resolve()[0], color)          # the chain only read the raster's colour
    inp = dict(src=color, depth=depth, vel=vel)
    pure = R.ref_multi_pass_frame(inp)
    print(f"380x280 after the raster: {int((want != pure).sum())} bytes differ from the restatement's own chain")
    assert not np.array_equal(want, color)


# ---- rejections --------------------------------------------------------------------------------------------------------------

def _p(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


def _overlapping(src):
    """(src copy, dst) in one allocation, dst one pixel further on."""
    buf = np.zeros(src.size + 4, np.uint8)
    a = buf[:src.size].reshape(src.shape)
    a[...] = src
    return a, buf[4:].reshape(src.shape)


REJECTIONS = ["vblur-nan", "vblur-width", "vblur-flags", "vblur-overlap", "vblur-null", "fog-nan", "fog-inf-power", "fog-end-is-start",
              "fog-span-overflows", "fog-height", "outline-radius-neg", "outline-radius-cap", "outline-nan", "outline-overlap",
              "fxaa-nan", "fxaa-overlap", "fxaa-same", "bright-nan", "additive-inf", "flare-no-ghosts", "flare-nine-ghosts",
              "flare-nan-scale", "flare-inf-chroma", "flare-overlap", "frame-mode", "frame-fog", "frame-dof-radius", "frame-null",
              "glow-iterations", "glow-flare", "glow-size"]


@pytest.fixture(scope="module")
def fresh_results():
    """What a context that never saw a rejected call computes."""
    import shs_gpu
    inp = R.inputs(SWEEP)
    with shs_gpu.Context(0) as c:
        return dict(fog=c.canvas_fog(inp["src"], inp["depth"], prequant=True),
                    frame=c.canvas_multi_pass_frame(inp["src"], inp["depth"], inp["vel"]),
                    glow=c.canvas_glow_frame(inp["src"], inp["depth"], inp["vel"], inp["spec"], bloom_iterations=2))


@pytest.mark.parametrize("what", REJECTIONS)
def test_rejected_inputs_leave_the_context_untouched(ctx, fresh_results, what):
    from shs_gpu import ShsError
    w, h = SWEEP
    inp = R.inputs(SWEEP)
    src, depth, vel, spec = inp["src"], inp["depth"], inp["vel"], inp["spec"]
    out = np.full_like(src, 7)
    L, H_ = ctx._lib, ctx._h
    nan, inf = float("nan"), float("inf")
    flags = 2 if what.endswith("flags") else 0
    s_in, s_out = _overlapping(src) if what.endswith("overlap") else (src, out)
    if what == "fxaa-same":
        s_in = s_out = src.copy()
    kind = what.split("-")[0]
    if kind == "vblur":
        d = ctx.fx_desc("velocity_blur", 0 if what == "vblur-width" else w, h, dict(strength=nan) if what == "vblur-nan" else None)
        rc = L.shs_canvas_velocity_blur(H_, ctypes.byref(d), _p(s_in), None if what == "vblur-null" else _p(vel), _p(s_out), flags)
    elif kind == "fog":
        p = {"fog-nan": dict(fog_start=nan), "fog-inf-power": dict(fog_power=-inf), "fog-end-is-start": dict(fog_start=33.0, fog_end=33.0),
             "fog-span-overflows": dict(fog_start=-3e38, fog_end=3e38), "fog-height": {}}[what]
        d = ctx.fx_desc("fog", w, -1 if what == "fog-height" else h, p)
        rc = L.shs_canvas_fog(H_, ctypes.byref(d), _p(src), _p(depth), _p(out), None, 0)
    elif kind == "outline":
        p = {"outline-radius-neg": dict(radius=-1), "outline-radius-cap": dict(radius=5), "outline-nan": dict(threshold=nan),
             "outline-overlap": {}}[what]
        rc = L.shs_canvas_outline(H_, ctypes.byref(ctx.fx_desc("outline", w, h, p)), _p(s_in), _p(depth), _p(s_out), 0)
    elif kind == "fxaa":
        d = ctx.fx_desc("fxaa", w, h, dict(span_max=nan) if what == "fxaa-nan" else None)
        rc = L.shs_canvas_fxaa(H_, ctypes.byref(d), _p(s_in), _p(s_out), 0)
    elif kind == "bright":
        rc = L.shs_canvas_spec_bright(H_, ctypes.byref(ctx.fx_desc("spec_bright", w, h, dict(intensity=nan))), _p(spec), _p(out), 0)
    elif kind == "additive":
        rc = L.shs_canvas_additive(H_, w, h, _p(src), _p(src), inf, _p(out), 0)
    elif kind == "flare":
        d = ctx.fx_desc("lens_flare", w, h, {"flare-nan-scale": dict(ghost_scales=(0.5, nan)), "flare-inf-chroma": dict(chroma_shift_px=inf)}.get(what))
        if what == "flare-no-ghosts":
            d.n_ghosts = 0
        if what == "flare-nine-ghosts":
            d.n_ghosts = 9
        rc = L.shs_canvas_lens_flare(H_, ctypes.byref(d), _p(s_in), _p(s_out), None, 0)
    elif kind == "frame":
        d = ctx.multi_pass_frame_desc(w, h)
        if what == "frame-mode":
            d.blur_mode = 3
        elif what == "frame-fog":
            d.fog.fog_end = d.fog.fog_start
        elif what == "frame-dof-radius":
            d.dof.autofocus_radius = 33
        rc = L.shs_canvas_multi_pass_frame(H_, ctypes.byref(d), _p(src), _p(depth), _p(vel), None if what == "frame-null" else _p(out), 0)
    else:
        d = ctx.glow_frame_desc(w, h)
        if what == "glow-iterations":
            d.bloom_iterations = -1
        elif what == "glow-flare":
            d.lens_flare.halo_intensity = nan
        else:
            d.width = 40000
        rc = L.shs_canvas_glow_frame(H_, ctypes.byref(d), _p(src), _p(depth), _p(vel), _p(spec), _p(out), 0)
    assert rc == -1
    assert (out == 7).all() and (what == "fxaa-same" or np.array_equal(s_in, src))
    with pytest.raises(ShsError):
        ctx._check(rc)
    fog = ctx.canvas_fog(src, depth, prequant=True)
    assert np.array_equal(fog[0], fresh_results["fog"][0]) and np.array_equal(fog[1].view(np.uint32), fresh_results["fog"][1].view(np.uint32))
    assert np.array_equal(ctx.canvas_multi_pass_frame(src, depth, vel), fresh_results["frame"])
    assert np.array_equal(ctx.canvas_glow_frame(src, depth, vel, spec, bloom_iterations=2), fresh_results["glow"])


def test_disabled_steps_are_not_checked(ctx):
    """A disabled DoF, FXAA, bloom or flare is not run, so its parameters are not judged."""
    inp = R.inputs(SWEEP)
    d_ok = ctx.canvas_multi_pass_frame(inp["src"], inp["depth"], inp["vel"], enable_dof=False, enable_fxaa=False)
    got = ctx.canvas_multi_pass_frame(inp["src"], inp["depth"], inp["vel"], enable_dof=False, enable_fxaa=False,
                                      dof=dict(radius=99), fxaa=dict(span_max=float("nan")))
    assert np.array_equal(got, d_ok)
