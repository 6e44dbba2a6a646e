"""The two passes of hello_ibl_skybox_optimized.cpp / hello_ibl_skybox_xsimd.cpp (shs_rt_render_ibl_phong, shading 11;
shs_rt_render_shadow_edge) and those demos' whole frames (GPU box), at the size the last profiles used: 380x280 over a
512x512 shadow map, tile jobs of 160, the demos' three knob sets, the scene of tools/exp_canvas_rt.py (the floor, a
textured monkey standing in for the car, the monkey), a 64^2 irradiance map and a 128^2 prefiltered base with 6 mips
(seeded floats), a 512^2-per-face cubemap sky under the clamp encode.

  python tools/exp_canvas_rt_ibl_phong.py profiles/canvas_rt_ibl_phong.txt     # appends its lines to the file
  python tools/exp_canvas_rt_ibl_phong.py - trace                              # FRAMES frames without events, for a
                                                                               # `rocprofv3 --kernel-trace --stats -- python ...` run

One context on one stream.  After a clock ramp (RAMP frames) and WARM warm-up frames, FRAMES frames of, in stream order with a
device event between the steps: shs_rt_render_shadow; shs_rt_render_shadow_edge (8 lanes) on the same casters; the shading-11
PASS1; the shading-4 PASS1 (hello_ibl_skybox.cpp's: the same raster under the same cubemap sky) over the same map; then the
two whole frames, each shadow or edge shadow, shading 11 with its background pass, shs_canvas_motion_blur over
shs_rt_device_targets with the demos' MB_* constants.  The sky and the IBL are bound once: neither binding does device work
in the frames."""
import ctypes
import dataclasses
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "leisure-software-renderer_amd"), ROOT, os.path.join(ROOT, "tools")]
import exp_canvas_rt as hard  # noqa: E402

FRAMES, WARM, RAMP = hard.FRAMES, hard.WARM, hard.RAMP
W, H, TILE, SM = 380, 280, 160, 512
FACE, IRR, SPEC, MIPS, LANES = 512, 64, 128, 6, 8
STEPS = ("shs_rt_render_shadow (k_rt_setup<1> + k_rt_raster<1, 0>)", "shs_rt_render_shadow_edge, 8 lanes (k_rt_setup_edge + k_rt_raster<1, 1>)",
         "PASS1 shading 11 (k_rt_setup<0> + k_rt_raster<0, 12> + k_rt_sky)", "PASS1 shading 4 (k_rt_setup<0> + k_rt_raster<0, 6> + k_rt_sky)",
         "whole frame, hello_ibl_skybox_optimized.cpp (shadow, shading 11, sky, blur)",
         "whole frame, hello_ibl_skybox_xsimd.cpp (edge shadow, shading 11, sky, blur)")


def frames_of(k):
    frame, draws = hard.demo(0.2 * (k + 1), 0.2 * k)
    frame = dataclasses.replace(frame, width=W, height=H, ref_tile=(TILE, TILE))   # (the same 4:3-ish projection)
    return dataclasses.replace(frame, shading=11), dataclasses.replace(frame, shading=4), draws


def summary(t_):
    q = statistics.quantiles(t_, n=4)
    return f"median {statistics.median(t_):.1f} us, mean {statistics.fmean(t_):.1f} us, quartiles {q[0]:.1f} .. {q[2]:.1f}, min {min(t_):.1f}, max {max(t_):.1f}"


def main():
    import numpy as np
    import torch

    import shs_gpu
    from shs_gpu import _abi, scene
    out = sys.argv[1] if len(sys.argv) > 1 else "-"
    mode = sys.argv[2] if len(sys.argv) > 2 else "both"
    ctx = shs_gpu.Context(0)
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    ctx.set_stream(stream.cuda_stream)
    rng = np.random.default_rng(1)
    faces = tuple(ctx.upload_texture(hard.Texture(rng.integers(0, 256, (FACE, FACE, 4), dtype=np.uint8))) for _ in range(6))
    cam = dict(cam_forward=(0.0, 0.0, 1.0), cam_right=(1.0, 0.0, 0.0), cam_up=(0.0, 1.0, 0.0), fov_degrees=60.0)
    ctx.rt_set_sky(shs_gpu.RtSky(model=2, encode=1, intensity=1.0, face_tex=faces, **cam))
    irr = rng.uniform(0.0, 2.0, (6, IRR, IRR, 3)).astype(np.float32)
    spec = [rng.uniform(0.0, 2.0, (6, max(1, SPEC >> m), max(1, SPEC >> m), 3)).astype(np.float32) for m in range(MIPS)]
    ctx.rt_set_ibl(irr, spec)
    # hello_ibl_skybox_optimized.cpp:1737-1741 (floor), :1805-1809 (car), :1862-1866 (monkey)
    phong = [shs_gpu.RtIblPhongDraw(0.30, 0.20, 0.04, 0.08, 32.0), shs_gpu.RtIblPhongDraw(0.28, 0.45, 0.04, 0.70, 96.0),
             shs_gpu.RtIblPhongDraw(0.30, 0.28, 0.04, 0.35, 48.0)]
    sky4 = [shs_gpu.RtSkyboxIblDraw(0.30, 0.22, 0.04, 0.10), shs_gpu.RtSkyboxIblDraw(0.28, 0.38, 0.04, 0.60),
            shs_gpu.RtSkyboxIblDraw(0.30, 0.32, 0.04, 0.35)]
    dst = torch.empty((H, W, 4), dtype=torch.uint8, device="cuda")
    _, proj = scene.camera((0.0, 10.0, -42.0), 0.0, 0.0)
    _P = ctypes.c_void_p

    def blur(frame):
        c_dev, d_dev, v_dev = ctx.rt_device_targets()
        md = _abi.CanvasMotionBlurDescC()
        md.width, md.height = W, H
        for k in range(16):
            md.curr_view[k] = md.prev_view[k] = float(frame.view[k])
            md.curr_proj[k] = md.prev_proj[k] = float(proj[k])
        md.samples, md.strength, md.w_obj, md.w_cam, md.soft_knee, md.knee_px, md.max_px = 12, 0.85, 1.0, 0.35, 1, 18.0, 22.0
        ctx._check(ctx._lib.shs_canvas_motion_blur(ctx._h, ctypes.byref(md), _P(c_dev), _P(d_dev), _P(v_dev), _P(dst.data_ptr()),
                                                   ctx.CANVAS_DEVICE))

    def one(k, ev=None):
        f11, f4, draws = frames_of(k)
        tile = (TILE, TILE)
        mark = (lambda i: ev[i].record(stream)) if ev else (lambda i: None)
        mark(0)
        ctx.rt_render_shadow(SM, f11.light_vp, draws, ref_tile=tile)
        mark(1)
        ctx.rt_render_shadow_edge(SM, f11.light_vp, draws, ref_tile=tile, lanes=LANES)
        mark(2)
        ctx.rt_render_ibl_phong(f11, draws, phong)
        mark(3)
        ctx.rt_render_skybox_ibl(f4, draws, sky4)
        mark(4)
        ctx.rt_render_shadow(SM, f11.light_vp, draws, ref_tile=tile)
        ctx.rt_render_ibl_phong(f11, draws, phong)
        blur(f11)
        mark(5)
        ctx.rt_render_shadow_edge(SM, f11.light_vp, draws, ref_tile=tile, lanes=LANES)
        ctx.rt_render_ibl_phong(f11, draws, phong)
        blur(f11)
        mark(6)

    for k in range(RAMP + WARM):
        one(k)
    ctx.synchronize()
    if mode == "trace":
        for k in range(FRAMES):
            one(k)
        ctx.synchronize()
        return
    evs = [[torch.cuda.Event(enable_timing=True) for _ in range(7)] for _ in range(FRAMES)]
    for k in range(FRAMES):
        one(k, evs[k])
    ctx.synchronize()
    st = ctx.rt_stats()
    shaded = int((ctx.rt_resolve_ids() >= 0).sum())
    lines = [f"exp_canvas_rt_ibl_phong: {W}x{H} tile {TILE}, map {SM}^2, irradiance {IRR}^2, specular {SPEC}^2 x {MIPS} mips, cubemap {FACE}^2 "
             f"per face, {st['input_tris']} triangles ({st}), {shaded} shaded pixels, {FRAMES} frames after {RAMP}+{WARM}"]
    med = []
    for i, name in enumerate(STEPS):
        t_ = [e[i].elapsed_time(e[i + 1]) * 1e3 for e in evs]
        med.append(statistics.median(t_))
        lines.append(f"  {name}: {summary(t_)}")
    lines.append(f"  edge shadow over shadow: {med[1] - med[0]:+.1f} us ({med[1] / med[0]:.3f}x); shading 11 over shading 4: "
                 f"{med[2] - med[3]:+.1f} us ({med[2] / med[3]:.3f}x), {1e3 * (med[2] - med[3]) / max(shaded, 1):.3f} ns per shaded pixel")
    text = "\n".join(lines)
    print(text)
    if out != "-":
        with open(os.path.join(ROOT, out) if not os.path.isabs(out) else out, "a") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
