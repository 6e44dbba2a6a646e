"""The HIP library path against the COMPILED REFERENCE (oracle/_ref/libshs_ref_lib.so: the reference
library's own rasterize_mesh / builtin programs / PCF / PassTonemap / PassMotionBlur over a GLM stand-in)
on the GPU rows of the uniform sweep (tests/lib_ref_cases.py), through the C ABI.

Depth and the triangle counters: bit-exact.  Motion and HDR: helpers.assert_float_close at its 1e-5,
absolute.  Every row's reference HDR stays below 8.0 (cases.GPU_HDR_CAP; asserted, never masked): the rows
above it are compared on the CPU only (tests/test_lib_reference.py).  Frames are 96x64, shadow maps at most
64^2, one context for the file."""
import numpy as np
import pytest

import lib_ref_cases as cases
from helpers import assert_depth_bitexact, assert_float_close

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ref(oracle_mod):
    if oracle_mod.reference_lib() is None:
        pytest.skip("neither oracle/_ref/libshs_ref_lib.so nor the reference tree to build it from is present")
    return oracle_mod


def _upload(dst, arr):
    """hipMemcpy of a host array into a device target of the context (no second GPU framework in the test)."""
    import ctypes
    hip = ctypes.CDLL("libamdhip64.so.7")   # by SONAME: the runtime already mapped (shs_gpu._abi.load)
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    arr = np.ascontiguousarray(arr)
    rc = hip.hipMemcpy(ctypes.c_void_p(dst), ctypes.c_void_p(arr.ctypes.data), arr.nbytes, 1)   # hipMemcpyHostToDevice
    assert rc == 0, rc


@pytest.mark.parametrize("row", cases.SWEEP_GPU, ids=[r["name"] for r in cases.SWEEP_GPU])
def test_sweep_vs_reference(gpu_ctx, ref, row):
    frame, draws, shadow = cases.sweep_scene(row)
    sm_ref = None
    if shadow is not None:
        lvp = gpu_ctx.render_shadow_map(*shadow)
        sm_ref, lvp_ref = ref.shadow_map(*shadow)
        assert np.array_equal(lvp.view(np.uint32), lvp_ref.view(np.uint32)), "light camera differs"
        assert_depth_bitexact(gpu_ctx.resolve_shadow_map(), sm_ref)
        cases.wire(row, draws, lvp)
    rh, rd, rm, rst = ref.ref_pbr_forward(frame, draws, sm_ref)
    peak = float(np.abs(rh).max())
    print(f"{row['name']}: reference |HDR| max {peak:.4f}")
    assert np.isfinite(rh).all() and peak < cases.GPU_HDR_CAP
    gpu_ctx.render_pbr_forward(frame, draws)
    gh, gd, gm = gpu_ctx.resolve_lib()
    st = gpu_ctx.lib_stats()
    for k in ("tri_input", "tri_after_clip", "tri_raster"):
        assert st[k] == rst[k], (k, st[k], rst[k])
    covered = int((rd < 1.0).sum())
    assert covered > 0 and rst["tri_after_clip"] > 0 and st["covered_pixels"] == covered
    assert_depth_bitexact(gd, rd)
    assert_float_close(gm, rm, what="motion")
    assert_float_close(gh, rh, what="hdr")


def test_tonemap_vs_reference(gpu_ctx, ref):
    """test_post.py's synthetic HDR target (every byte boundary, NaN, +-inf, negative, denormal, huge)
    written into the device HDR target: the bytes of the reference's PassTonemap."""
    from shs_gpu import scene_lib
    hdr = cases.synthetic_hdr(256, 64)
    frame, draws, _, _, _ = scene_lib.c5_scene(256, 64)
    ctx = gpu_ctx
    ctx.render_pbr_forward(frame, draws)
    ctx.synchronize_lib()
    _upload(ctx.lib_device_targets()[0], hdr)
    ctx.tonemap(1.0, 2.2)
    ldr, _ = ctx.resolve_ldr()
    want = ref.ref_tonemap(hdr, 1.0, 2.2)
    bad = np.argwhere(ldr != want)
    assert bad.size == 0, f"{len(bad)} mismatches, first {bad[:4]}"
    assert len(np.unique(want[..., :3])) == 256


def test_motion_blur_vs_reference(gpu_ctx, ref):
    """test_post.py's non-finite motion plane over a rendered 160x96 frame: the bytes of the reference's
    PassMotionBlur."""
    from shs_gpu import scene_lib
    frame, draws, _, _, _ = scene_lib.c5_scene(160, 96)
    mot = cases.nonfinite_motion(160, 96)
    ctx = gpu_ctx
    ctx.render_pbr_forward(frame, draws)
    ctx.synchronize_lib()
    _upload(ctx.lib_device_targets()[2], mot)
    ctx.tonemap(1.0, 2.2, ldr=True, present=False)
    ctx.motion_blur(min_velocity_px=0.0)
    got, _ = ctx.resolve_motion_blur()
    ldr, _ = ctx.resolve_ldr()
    _, depth, motion = ctx.resolve_lib()
    assert np.array_equal(motion.view(np.uint32), mot.view(np.uint32)), "injected motion was overwritten"
    want = ref.ref_motion_blur(ldr, depth, motion, min_velocity_px=0.0)
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{len(bad)} byte mismatches, first {bad[:4]}"
    assert not np.array_equal(want, ldr), "blur changed nothing"
