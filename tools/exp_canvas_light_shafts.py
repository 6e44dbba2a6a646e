"""The light-shafts pass (shs_canvas_light_shafts, PASS1.5 of hello_pbr_light_shafts.cpp) on that demo's frame (GPU box):
800x600, tile jobs of 160, a 1024x1024 shadow map, the demo's LightShaftParams; the scene, camera, light, IBL and materials
are tools/exp_canvas_rt_pbr.py's.

  python tools/exp_canvas_light_shafts.py profiles/canvas_light_shafts.txt   # appends its lines to the file
  python tools/exp_canvas_light_shafts.py - trace                            # FRAMES frames without events, for a
                                                                             # `rocprofv3 --kernel-trace --stats -- python ...` run

One context on one stream; a frame is the demo's chain without a host round trip: PASS0 (shs_rt_render_shadow), PASS1
(shs_rt_render_pbr, shading 2: the GGX + IBL shader under the 2x2 PCF), PASS1.5 (the light shafts over shs_rt_device_targets
and shs_rt_device_shadow_map, in place) and PASS2 (shs_canvas_motion_blur).  After a clock ramp (RAMP frames) and WARM
warm-up frames it times FRAMES frames with device events around PASS1, PASS1.5 and PASS2, so the three are measured in
the same run under the same clocks."""
import ctypes
import dataclasses
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "leisure-software-renderer_amd"), ROOT, os.path.join(ROOT, "tools")]
import exp_canvas_rt_pbr as pbr  # noqa: E402

FRAMES, WARM, RAMP = pbr.FRAMES, pbr.WARM, pbr.RAMP
W, H, TILE, SM = 800, 600, 160, 1024
CAM = (0.0, 10.0, -42.0)     # exp_canvas_rt.demo's camera


def main():
    import numpy as np
    import torch

    import shs_gpu
    from shs_gpu import _abi, scene
    out = sys.argv[1] if len(sys.argv) > 1 else "-"
    trace = len(sys.argv) > 2 and sys.argv[2] == "trace"
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    ctx = shs_gpu.Context(0)
    ctx.set_stream(stream.cuda_stream)
    ctx.rt_set_ibl(*pbr.make_ibl())
    view, proj = scene.camera(CAM, 0.0, 0.0)
    vp = np.asarray(scene.mat_mul(proj, view), np.float64).reshape(4, 4).T
    inv_vp = np.ascontiguousarray(np.linalg.inv(vp).T).reshape(16).astype(np.float32)
    blurred = torch.empty((H, W, 4), dtype=torch.uint8, device="cuda")
    _P = ctypes.c_void_p

    def descs(frame):
        d = _abi.CanvasLightShaftsDescC()
        d.width, d.height, d.shadow_w, d.shadow_h = W, H, SM, SM
        for k in range(3):
            d.cam_pos[k], d.sun_dir_world[k] = float(CAM[k]), float(frame.light_dir_world[k])
        for k in range(16):
            d.inv_view_proj[k], d.light_vp[k] = float(inv_vp[k]), float(np.asarray(frame.light_vp).reshape(16)[k])
        for name, ctype in _abi.CanvasLightShaftsDescC._fields_[8:]:
            v = shs_gpu.Context.LIGHT_SHAFTS_DEFAULTS[name]
            setattr(d, name, int(v) if ctype is ctypes.c_int32 else float(v))
        m = _abi.CanvasMotionBlurDescC()
        m.width, m.height = W, H
        for k in range(16):
            m.curr_view[k] = m.prev_view[k] = float(view[k])
            m.curr_proj[k] = m.prev_proj[k] = float(proj[k])
        m.samples, m.strength, m.w_obj, m.w_cam, m.soft_knee, m.knee_px, m.max_px = 12, 0.85, 1.0, 0.35, 1, 18.0, 22.0
        return d, m

    def one(k, ev=None):
        frame, _, draws, mats = pbr.frames_of(k)
        frame = dataclasses.replace(frame, width=W, height=H, ref_tile=(TILE, TILE))
        d, m = descs(frame)
        ctx.rt_render_shadow(SM, frame.light_vp, draws, ref_tile=(TILE, TILE))
        if ev:
            ev[0].record(stream)
        ctx.rt_render_pbr(frame, draws, mats)
        color, depth, vel = ctx.rt_device_targets()
        smap, _ = ctx.rt_device_shadow_map()
        if ev:
            ev[1].record(stream)
        ctx._check(ctx._lib.shs_canvas_light_shafts(ctx._h, ctypes.byref(d), _P(color), _P(depth), _P(smap), _P(color), None,
                                                    ctx.CANVAS_DEVICE))
        if ev:
            ev[2].record(stream)
        ctx._check(ctx._lib.shs_canvas_motion_blur(ctx._h, ctypes.byref(m), _P(color), _P(depth), _P(vel), _P(blurred.data_ptr()),
                                                   ctx.CANVAS_DEVICE))
        if ev:
            ev[3].record(stream)

    for k in range(RAMP + WARM):
        one(k)
    ctx.synchronize()
    if trace:
        for k in range(FRAMES):
            one(k)
        ctx.synchronize()
        return
    evs = [[torch.cuda.Event(enable_timing=True) for _ in range(4)] for _ in range(FRAMES)]
    for k in range(FRAMES):
        one(k, evs[k])
    ctx.synchronize()
    depth = ctx.rt_resolve()[1]
    covered = int((depth < np.finfo(np.float32).max).sum())
    lines = [f"exp_canvas_light_shafts: {W}x{H} tile {TILE}, map {SM}^2, {covered} covered pixels of {W * H}, 40 steps, "
             f"{FRAMES} frames after {RAMP}+{WARM}"]
    for name, j in (("PASS1 pbr (shading 2)", 0), ("PASS1.5 light shafts", 1), ("PASS2 motion blur", 2)):
        t = [e[j].elapsed_time(e[j + 1]) * 1e3 for e in evs]
        lines.append(f"  {name}: median {statistics.median(t):.1f} us, mean {statistics.fmean(t):.1f} us, min {min(t):.1f}, max {max(t):.1f}")
    text = "\n".join(lines)
    print(text)
    if out != "-":
        with open(os.path.join(ROOT, out) if not os.path.isabs(out) else out, "a") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
