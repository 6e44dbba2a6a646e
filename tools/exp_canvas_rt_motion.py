"""The unclipped camera pass (shs_rt_render_motion, shadings 6 and 7) and the three demos' whole frames on the GPU box, at
the demos' 380x280 canvas: hello_multi_pass.cpp (three monkeys, tile jobs of 80, 40 px; chain blur mode 0),
hello_camera_and_perobject_motion_blur.cpp's order (blur mode 2, 22 px) and hello_glowing_star.cpp (a 40-triangle star, one
job covering the frame, 30 px; the glow chain over the spec plane).

  python tools/exp_canvas_rt_motion.py profiles/canvas_rt_motion.txt   # appends its lines to the file
  python tools/exp_canvas_rt_motion.py - trace                         # FRAMES frames of each demo without events, for a
                                                                       # `rocprofv3 --kernel-trace --stats -- python ...` run:
                                                                       # k_rt_setup_motion's and k_rt_raster<false, 8 / 9>'s
                                                                       # own durations

One context on one stream; every call goes straight to the C entry with the frame, the draw table and the descs built
once, so the host adds a ctypes call per entry and nothing else.  After a clock ramp (RAMP frames) and WARM warm-up
frames, FRAMES frames of: the raster (draw-table upload, counter clear, k_rt_setup_motion, k_rt_raster), then the demo's
chain over shs_rt_device_targets (and shs_rt_device_spec) with SHS_CANVAS_DEVICE.  A device event before the raster,
between the two and after the chain: what each costs in a stream of dependent launches, not the kernels alone."""
import ctypes
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "leisure-software-renderer_amd"), ROOT]

W, H = 380, 280
FRAMES, WARM, RAMP = 200, 20, 60


def star_mesh():
    """A ten-point star prism with raised cap centres: 40 flat-shaded triangles wound outward."""
    import numpy as np
    from shs_gpu import scene
    ang = np.radians(90.0) + np.arange(10) * np.radians(36.0)
    rad = np.where(np.arange(10) % 2 == 0, 1.0, 0.5)
    ring = np.stack([np.cos(ang) * rad, np.sin(ang) * rad], 1)
    tris = []
    for i in range(10):
        j = (i + 1) % 10
        a0, a1, b0, b1 = (*ring[i], -0.25), (*ring[j], -0.25), (*ring[i], 0.25), (*ring[j], 0.25)
        tris += [((0, 0, -0.55), a0, a1), ((0, 0, 0.55), b1, b0), (a0, b0, b1), (a0, b1, a1)]
    pos, nrm = [], []
    for t in np.asarray(tris, np.float64):
        n = np.cross(t[1] - t[0], t[2] - t[0])
        if np.dot(n, t.mean(0)) < 0:
            t, n = t[[0, 2, 1]], -n
        pos.append(t.reshape(9))
        nrm.append(np.tile(n / np.linalg.norm(n), 3))
    return scene.Mesh(np.array(pos, np.float32), np.array(nrm, np.float32), None)


def demo(which):
    """-> (RtFrame, [RtDraw]) of 'multi' (shading 6) or 'star' (shading 7)."""
    import numpy as np
    import shs_gpu
    from shs_gpu import lib_path, scene
    eye = np.eye(4, dtype=np.float32).reshape(16)
    if which == "star":
        cam, target, light = (0.0, 0.5, -2.3), (0.0, 0.5, 0.0), (0.3, -0.4, 1.0)
    else:
        cam, target, light = (0.0, 4.0, -9.0), (0.0, 0.5, 0.0), (-0.45, -1.0, 0.55)
    view = lib_path.look_at_lh(cam, target)
    vp = scene.mat_mul(lib_path.perspective_lh_no(float(np.radians(60.0)), W / H, 0.1, 100.0), view)

    def draw(mesh, model, prev, color):
        return shs_gpu.RtDraw(mesh, model, scene.mat_mul(vp, model), scene.mat_mul(vp, prev), color)
    if which == "star":
        draws = [draw(star_mesh(), scene.model_trs((0.0, 0.5, 0.0), 25.0, (1.0,) * 3), scene.model_trs((0.15, 0.5, 0.0), 13.0, (1.0,) * 3),
                      (240, 200, 60, 255))]
        tile, max_px, shading = (W, H), 30.0, 7
    else:
        s = (1.8, 1.8, 1.8)
        m = scene.monkey()
        draws = [draw(m, scene.model_trs((-3.5, 1.5, 3.0), 20.0, s), scene.model_trs((-3.5, 1.5, 3.0), 8.0, s), (60, 100, 200, 255)),
                 draw(m, scene.model_trs((0.0, 1.2, 1.0), -30.0, s), scene.model_trs((5.5, 1.2, 1.0), -30.0, s), (200, 90, 80, 255)),
                 draw(m, scene.model_trs((3.5, 1.8, 4.5), 200.0, s), scene.model_trs((3.5, 1.8, 4.5), 200.0, s), (80, 200, 120, 255))]
        tile, max_px, shading = (80, 80), 40.0, 6
    frame = shs_gpu.RtFrame(W, H, view, eye, light, cam, ref_tile=tile, max_velocity_px=max_px, use_shadow=False, pcf=False, shading=shading)
    return frame, draws, view


def summary(t_):
    q = statistics.quantiles(t_, n=4)
    return f"median {statistics.median(t_):.1f} us, mean {statistics.fmean(t_):.1f} us, quartiles {q[0]:.1f} .. {q[2]:.1f}, min {min(t_):.1f}, max {max(t_):.1f}"


def main():
    import torch

    import shs_gpu
    from shs_gpu import lib_path
    out = sys.argv[1] if len(sys.argv) > 1 else "-"
    trace = len(sys.argv) > 2 and sys.argv[2] == "trace"
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    ctx = shs_gpu.Context(0)
    ctx.set_stream(stream.cuda_stream)
    L, DEV, ref, P = ctx._lib, ctx.CANVAS_DEVICE, ctypes.byref, ctypes.c_void_p
    dst = torch.empty((H, W, 4), dtype=torch.uint8, device="cuda")
    lines = [f"exp_canvas_rt_motion: {W}x{H}, {FRAMES} frames after {RAMP}+{WARM}; us per frame of a back-to-back stream"]
    import numpy as np
    proj = lib_path.perspective_lh_no(float(np.radians(60.0)), W / H, 0.1, 100.0)
    for name, which, mode in (("hello_multi_pass.cpp", "multi", 0), ("hello_camera_and_perobject_motion_blur.cpp", "multi", 2),
                              ("hello_glowing_star.cpp", "star", None)):
        frame, draws, view = demo(which)
        if mode == 2:
            frame.max_velocity_px = 22.0
        fc, arr, n = ctx._rt_frame_c(frame), ctx._rt_draw_array(draws), len(draws)
        if which == "star":
            desc = ctx.glow_frame_desc(W, H)
        else:
            cam = dict(curr_view=view, curr_proj=proj, prev_view=lib_path.look_at_lh((0.3, 4.1, -8.8), (0.1, 0.5, 0.0)), prev_proj=proj)
            desc = ctx.multi_pass_frame_desc(W, H, mode, **(dict(motion_blur=cam) if mode else {}))

        def one(ev=None):
            if ev:
                ev[0].record(stream)
            ctx._check(L.shs_rt_render_motion(ctx._h, ref(fc), arr, n))
            if ev:
                ev[1].record(stream)
            c, d, v = ctx.rt_device_targets()
            if which == "star":
                ctx._check(L.shs_canvas_glow_frame(ctx._h, ref(desc), P(c), P(d), P(v), P(ctx.rt_device_spec()), P(dst.data_ptr()), DEV))
            else:
                ctx._check(L.shs_canvas_multi_pass_frame(ctx._h, ref(desc), P(c), P(d), P(v), P(dst.data_ptr()), DEV))
            if ev:
                ev[2].record(stream)
        for _ in range(RAMP + WARM):
            one()
        ctx.synchronize()
        if trace:
            for _ in range(FRAMES):
                one()
            ctx.synchronize()
            continue
        evs = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(FRAMES)]
        for k in range(FRAMES):
            one(evs[k])
        ctx.synchronize()
        ctx._rt_size = (W, H)      # (the C entry was called directly: tell the wrapper what there is to resolve)
        st = ctx.rt_stats()
        shown = int((ctx.rt_resolve_ids() >= 0).sum())
        lines.append(f"  {name}: shading {frame.shading}, tile {frame.ref_tile}, {st['input_tris']} triangles of which {st['sub_tris']} kept, "
                     f"{shown} shown pixels of {W * H}")
        lines.append(f"    raster (upload, clear, setup, raster): {summary([e[0].elapsed_time(e[1]) * 1e3 for e in evs])}")
        lines.append(f"    chain over the device planes:          {summary([e[1].elapsed_time(e[2]) * 1e3 for e in evs])}")
        lines.append(f"    whole frame, all on the device:        {summary([e[0].elapsed_time(e[2]) * 1e3 for e in evs])}")
    text = "\n".join(lines)
    print(text)
    if out != "-" and not trace:
        with open(os.path.join(ROOT, out) if not os.path.isabs(out) else out, "a") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
