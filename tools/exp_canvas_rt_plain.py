"""The three plain demos' whole frames (shs_rt_render_plain, shadings 8 to 10, and each demo's post pass) on the GPU box at
the demos' 380x280 canvas, beside the shading-6 raster (shs_rt_render_motion) of the same geometry in the same run:
tools/exp_canvas_rt_motion.py's three monkeys under tile jobs of 80.

  python tools/exp_canvas_rt_plain.py profiles/canvas_rt_plain.txt   # appends its lines to the file
  python tools/exp_canvas_rt_plain.py - trace                        # FRAMES frames of each without events, for a
                                                                     # `rocprofv3 --kernel-trace --stats -- python ...` run

One context on one stream; every call goes straight to the C entry with the frame, the draw table and the descs built
once.  After a clock ramp (RAMP frames) and WARM warm-up frames, FRAMES frames of: the raster (draw-table upload, counter
clear, k_rt_setup_motion, k_rt_raster), then the demo's post pass over shs_rt_device_targets with SHS_CANVAS_DEVICE --
shs_canvas_object_blur with depth_rows 1 (hello_per_object_motion_blur.cpp), shs_canvas_dof without the focus read-back
(hello_depth_of_field.cpp), shs_canvas_ping_pong_blur with three iterations (hello_ping_pong.cpp).  A device event before
the raster, between the two and after the post pass: what each costs in a stream of dependent launches, not the kernels
alone.  Then the object blur alone: BATCH launches between one pair of events, RUNS times."""
import ctypes
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "leisure-software-renderer_amd"), ROOT, os.path.join(ROOT, "tools")]

W, H = 380, 280
FRAMES, WARM, RAMP = 200, 20, 60
BATCH, RUNS = 200, 8


def summary(t_):
    q = statistics.quantiles(t_, n=4)
    return f"median {statistics.median(t_):.1f} us, mean {statistics.fmean(t_):.1f} us, quartiles {q[0]:.1f} .. {q[2]:.1f}, min {min(t_):.1f}, max {max(t_):.1f}"


def main():
    import dataclasses

    import torch

    import exp_canvas_rt_motion as X
    import shs_gpu
    out = sys.argv[1] if len(sys.argv) > 1 else "-"
    trace = len(sys.argv) > 2 and sys.argv[2] == "trace"
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    ctx = shs_gpu.Context(0)
    ctx.set_stream(stream.cuda_stream)
    L, DEV, ref, P = ctx._lib, ctx.CANVAS_DEVICE, ctypes.byref, ctypes.c_void_p
    dst = torch.empty((H, W, 4), dtype=torch.uint8, device="cuda")
    lines = [f"exp_canvas_rt_plain: {W}x{H}, {FRAMES} frames after {RAMP}+{WARM}; us per frame of a back-to-back stream"]
    frame6, draws, _ = X.demo("multi")
    arr, n = ctx._rt_draw_array(draws), len(draws)
    blur_d = ctx.fx_desc("object_blur", W, H)
    dof_d = ctx.fx_desc("dof", W, H, dict(iterations=3, radius=6, range_=24.0, max_blur=0.6))
    for name, shading in (("hello_multi_pass.cpp's raster alone", 6), ("hello_per_object_motion_blur.cpp", 8), ("hello_depth_of_field.cpp", 9),
                          ("hello_ping_pong.cpp", 10)):
        frame = dataclasses.replace(frame6, shading=shading)
        fc = ctx._rt_frame_c(frame)
        render = L.shs_rt_render_motion if shading == 6 else L.shs_rt_render_plain

        def one(ev=None):
            if ev:
                ev[0].record(stream)
            ctx._check(render(ctx._h, ref(fc), arr, n))
            if ev:
                ev[1].record(stream)
            c, d, v = ctx.rt_device_targets()
            if shading == 8:
                ctx._check(L.shs_canvas_object_blur(ctx._h, ref(blur_d), P(c), P(d), P(v), P(dst.data_ptr()), DEV))
            elif shading == 9:
                ctx._check(L.shs_canvas_dof(ctx._h, ref(dof_d), P(c), P(d), None, None, DEV))
            elif shading == 10:
                ctx._check(L.shs_canvas_ping_pong_blur(ctx._h, W, H, 3, P(c), DEV))
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
        lines.append(f"  {name}: shading {shading}, tile {frame.ref_tile}, {st['input_tris']} triangles of which {st['sub_tris']} kept, "
                     f"{shown} shown pixels of {W * H}")
        lines.append(f"    raster (upload, clear, setup, raster): {summary([e[0].elapsed_time(e[1]) * 1e3 for e in evs])}")
        if shading != 6:
            lines.append(f"    post pass over the device planes:      {summary([e[1].elapsed_time(e[2]) * 1e3 for e in evs])}")
            lines.append(f"    whole frame, all on the device:        {summary([e[0].elapsed_time(e[2]) * 1e3 for e in evs])}")
    if not trace:
        # the object blur alone over a shading-8 frame's planes
        ctx._check(L.shs_rt_render_plain(ctx._h, ref(ctx._rt_frame_c(dataclasses.replace(frame6, shading=8))), arr, n))
        c, d, v = ctx.rt_device_targets()
        per = []
        for _ in range(RUNS + 1):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            for _ in range(BATCH):
                ctx._check(L.shs_canvas_object_blur(ctx._h, ref(blur_d), P(c), P(d), P(v), P(dst.data_ptr()), DEV))
            b.record(stream)
            ctx.synchronize()
            per.append(a.elapsed_time(b) * 1e3 / BATCH)
        ctx._rt_size = (W, H)
        vel = ctx.rt_resolve()[2]
        moving = int((((vel * 1.85) ** 2).sum(-1) >= 0.25).sum())
        lines.append(f"  shs_canvas_object_blur alone ({moving} of {W * H} pixels gather), us per launch of {BATCH} back to back, {RUNS} runs after one: "
                     f"{' '.join(f'{t:.2f}' for t in per[1:])}")
    text = "\n".join(lines)
    print(text)
    if out != "-" and not trace:
        with open(os.path.join(ROOT, out) if not os.path.isabs(out) else out, "a") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
