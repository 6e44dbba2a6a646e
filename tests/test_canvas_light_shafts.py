"""shs_canvas_light_shafts on the GPU (light_shafts_pass of hello_pbr_light_shafts.cpp, the PASS1.5 of that demo's frame)
against tests/canvas_light_shafts_ref (test_canvas_light_shafts_ref.py holds the wrapper, the inputs, the parameter
sets and what pins the reference on the CPU).

Everything before a transcendental is the reference's bits on the device too; its sin / cos / exp / pow are double
evaluations rounded once to float where the restatement calls the float libm.  So:

  * a pixel the restatement only copies keeps its four bytes and has (0, 0, 0, -1) in the prequant plane;
  * on marched pixels the number of accumulated steps (a density compared with 1e-6, a transmittance with 0.01) equals
    the restatement's, except on at most 1 in 2,000 of the frame's marched pixels, which are counted, printed and left out
    of the next two checks (the restatement against its own double variant stays within a quarter of that, on the CPU);
  * the bytes go through helpers.assert_color_parity and the pre-truncation floats are within helpers.TOL * 255."""
import ctypes

import numpy as np
import pytest

import helpers
import test_canvas_light_shafts_ref as L
import test_canvas_rt_ref as R
from test_canvas_rt_ref import F

pytestmark = pytest.mark.gpu
COPIED = np.array([0, 0, 0, -1], F)


@pytest.fixture(scope="module")
def ctx():
    import shs_gpu
    c = shs_gpu.Context(0)
    yield c
    c.close()


def _run(ctx, inp, params, shadow="own", **kw):
    sm = inp["shadow"] if isinstance(shadow, str) else shadow
    return ctx.canvas_light_shafts(inp["src"], inp["depth"], inp["cam_pos"], inp["inv_vp"], inp["sun"], inp["light_vp"], sm,
                                   params=params, prequant=True, **kw)


def _check(got_c, got_pq, inp, ref, label):
    ref_c, ref_pq = ref["color"], ref["pq"]
    m = L.marched(ref_pq)
    assert np.array_equal(got_c[~m], inp["src"][~m]), f"{label}: a copied pixel changed"
    assert np.array_equal(got_pq[~m], np.broadcast_to(COPIED, got_pq[~m].shape)), f"{label}: a copied pixel's prequant"
    assert (got_pq[..., 3][m] >= 0).all(), f"{label}: a marched pixel was copied"
    flips = m & (got_pq[..., 3] != ref_pq[..., 3])
    cap = L.step_cap(int(m.sum()))
    print(f"{label}: {int(flips.sum())} of {int(m.sum())} marched pixels differ in their step count (cap {cap})")
    assert int(flips.sum()) <= cap, f"{label}: step counts differ at {np.argwhere(flips)[:4].tolist()}"
    keep = ~flips
    n_bytes = helpers.assert_color_parity(got_c[keep], ref_c[keep], got_pq[keep], ref_pq[keep])
    g, r = got_pq[keep][:, :3], ref_pq[keep][:, :3]
    err = np.abs(g.astype(np.float64) - r.astype(np.float64))
    inexact = int((g.view(np.uint32) != r.view(np.uint32)).sum())
    print(f"{label}: {inexact} of {g.size} pre-truncation floats not bit-identical, largest difference {err.max():.3g} "
          f"(bar {helpers.TOL * 255:.3g}), {n_bytes} bytes off by one")
    assert err.max() <= helpers.TOL * 255.0, f"{label}: pre-truncation floats differ by {err.max()}"


@pytest.mark.parametrize("size", L.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", list(L.ALL_SETS))
def test_host_buffers_equal_the_restatement(ctx, name, size):
    inp, params, ref = L.case(name, size)
    got_c, got_pq = _run(ctx, inp, params)
    _check(got_c, got_pq, inp, ref, f"{name} {size[0]}x{size[1]}")


def test_non_square_map(ctx):
    inp, params, ref = L.case("demo", L.SIZES[1], L.MAP_SIZES[1])
    assert inp["shadow"].shape == (64, 96)
    got_c, got_pq = _run(ctx, inp, params)
    _check(got_c, got_pq, inp, ref, "demo 96x72, map 96x64")
    square = L.case("demo", L.SIZES[1])[2]
    assert not np.array_equal(square["color"], ref["color"])


def test_no_map_is_every_step_lit(ctx):
    inp = L.inputs(L.SIZES[1])
    ref = L.ref_pass(inp, {}, shadow=None)
    got_c, got_pq = _run(ctx, inp, {}, shadow=None)
    _check(got_c, got_pq, inp, ref, "demo 96x72, no map")


def test_device_tensors_in_place(ctx):
    """torch CUDA tensors, dst is src (a pixel reads only its own), the map a device tensor too."""
    import torch
    inp, params, ref = L.case("demo")
    src = torch.from_numpy(inp["src"].copy()).cuda()
    depth = torch.from_numpy(inp["depth"].copy()).cuda()
    sm = torch.from_numpy(inp["shadow"].copy()).cuda()
    out, pq = ctx.canvas_light_shafts(src, depth, inp["cam_pos"], inp["inv_vp"], inp["sun"], inp["light_vp"], sm, params=params,
                                      dst=src, prequant=True)
    assert out is src
    ctx.synchronize()
    _check(out.cpu().numpy(), pq.cpu().numpy(), inp, ref, "demo 160x120, device, in place")


def _desc_and_buffers(inp):
    d = L.make_desc(inp, {})
    out = np.zeros_like(inp["src"])
    return d, out


@pytest.mark.parametrize("what", ["width", "height", "steps", "nan-param", "inf-matrix", "nan-light", "nan-cam", "zero-sun",
                                  "map-size", "flags", "null-src"])
def test_rejected_inputs_leave_the_context_untouched(ctx, what):
    from shs_gpu import ShsError, _abi
    inp, params, _ = L.case("demo", L.SIZES[1])
    good_c, good_pq = _run(ctx, inp, params)
    d, out = _desc_and_buffers(inp)
    out[:] = 7
    flags, src = 0, inp["src"]
    if what == "width":
        d.width = 0
    elif what == "height":
        d.height = -3
    elif what == "steps":
        d.steps = _abi.CANVAS_LIGHT_SHAFTS_MAX_STEPS + 1
    elif what == "nan-param":
        d.sigma_t = float("nan")
    elif what == "inf-matrix":
        d.inv_view_proj[5] = float("inf")
    elif what == "nan-light":
        d.light_vp[0] = float("nan")
    elif what == "nan-cam":
        d.cam_pos[2] = float("-inf")
    elif what == "zero-sun":
        d.sun_dir_world[0] = d.sun_dir_world[1] = d.sun_dir_world[2] = 0.0
    elif what == "map-size":
        d.shadow_w = 0
    elif what == "flags":
        flags = 2
    _p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    rc = ctx._lib.shs_canvas_light_shafts(ctx._h, ctypes.byref(d), None if what == "null-src" else _p(src), _p(inp["depth"]),
                                          _p(inp["shadow"]), _p(out), None, flags)
    assert rc == -1
    assert (out == 7).all()
    with pytest.raises(ShsError):
        ctx._check(rc)
    again_c, again_pq = _run(ctx, inp, params)
    assert np.array_equal(again_c, good_c) and np.array_equal(again_pq.view(np.uint32), good_pq.view(np.uint32))


def test_steps_at_the_limit_and_below_one(ctx):
    """steps = 4096 is accepted; steps <= 0 marches one step, as std::max(1, p.steps)."""
    from shs_gpu import _abi
    inp = L.inputs(L.SIZES[1])
    for steps in (0, -5):
        p = dict(L.ALL_SETS["one_step"], steps=steps)
        ref = L.ref_pass(inp, p)
        got_c, got_pq = _run(ctx, inp, p)
        _check(got_c, got_pq, inp, ref, f"steps {steps}")
        assert np.array_equal(ref["pq"], L.case("one_step", L.SIZES[1])[2]["pq"])
    small = dict(L.inputs(L.SIZES[1]))
    small.update(w=32, h=8, src=np.ascontiguousarray(inp["src"][:8, :32]), depth=np.ascontiguousarray(inp["depth"][:8, :32]))
    p = dict(steps=_abi.CANVAS_LIGHT_SHAFTS_MAX_STEPS)
    got_c, got_pq = _run(ctx, small, p)
    _check(got_c, got_pq, small, L.ref_pass(small, p), "steps 4096, 32x8")


def test_rt_device_shadow_map_is_the_resolved_map(ctx):
    from shs_gpu import ShsError
    import shs_gpu
    fresh = shs_gpu.Context(0)
    try:
        with pytest.raises(ShsError):
            fresh.rt_device_shadow_map()
    finally:
        fresh.close()
    _, light_vp, draws = R.scene_demo()
    ctx.rt_render_shadow((96, 64), light_vp, draws)
    want = ctx.rt_resolve_shadow()
    ptr, (w, h) = ctx.rt_device_shadow_map()
    assert (w, h) == (96, 64) and ptr
    ctx.synchronize()
    got = np.empty((h, w), F)
    hip = ctypes.CDLL("libamdhip64.so.7")   # by SONAME: the runtime already mapped (shs_gpu._abi.load)
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    assert hip.hipMemcpy(ctypes.c_void_p(got.ctypes.data), ctypes.c_void_p(ptr), got.nbytes, 2) == 0   # hipMemcpyDeviceToHost
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(want.view(np.uint32), R.ref_shadow((96, 64), light_vp, draws).view(np.uint32))


def test_chain_after_the_raster_on_the_device(ctx):
    """PASS0 -> PASS1.5 without a resolve: the pass over device buffers with the raster's own device map equals the pass
    over the resolved map."""
    import torch
    inp, params, ref = L.case("demo", L.SIZES[0], L.MAP_SIZES[0])
    _, light_vp, draws = R.scene_demo()
    ctx.rt_render_shadow(L.MAP_SIZES[0], light_vp, draws)
    ptr, size = ctx.rt_device_shadow_map()
    src = torch.from_numpy(inp["src"].copy()).cuda()
    depth = torch.from_numpy(inp["depth"].copy()).cuda()
    out, pq = ctx.canvas_light_shafts(src, depth, inp["cam_pos"], inp["inv_vp"], inp["sun"], inp["light_vp"], ptr, shadow_size=size,
                                      params=params, prequant=True)
    ctx.synchronize()
    _check(out.cpu().numpy(), pq.cpu().numpy(), inp, ref, "demo 160x120 over rt_device_shadow_map")
