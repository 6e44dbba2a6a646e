"""The PCSS soft-shadow camera pass on hello_shadow_mapping_soft.cpp's own frame (GPU box): 800x600, tile jobs of
160, a 2048x2048 shadow map, the scene of tools/exp_canvas_rt.py (FloorPlane(55, 140) with 48x48 cells, the monkey
at the demo's transform and a second, textured monkey standing in for the car), the demo's PCSS constants.

  python tools/exp_canvas_rt_soft.py profiles/canvas_rt_soft.txt   # appends its lines to the file
  python tools/exp_canvas_rt_soft.py - trace                       # FRAMES frames without events, for a
                                                                   # `rocprofv3 --kernel-trace --stats -- python ...` run

After a clock ramp (RAMP frames) and WARM warm-up frames it times FRAMES frames with device events on the context
stream.  Each frame is PASS0, then the soft PASS1 (shading 1), then the hard PCF PASS1 (shading 0) of the same scene
and tile size over the same map, one event before each and one after the last: the two camera passes are measured
in the same run under the same clocks.  It also reports the first soft frame's host time (which builds and uploads
the per-pixel rotation table) beside a later one's, and the table's size."""
import dataclasses
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "leisure-software-renderer_amd"), ROOT, os.path.join(ROOT, "tools")]
import exp_canvas_rt as hard  # noqa: E402

FRAMES, WARM, RAMP = hard.FRAMES, hard.WARM, hard.RAMP
W, H, TILE, SM = 800, 600, 160, 2048


def frames_of(k):
    frame, draws = hard.demo(0.2 * (k + 1), 0.2 * k)
    frame = dataclasses.replace(frame, ref_tile=(TILE, TILE))
    return dataclasses.replace(frame, shading=1), frame, draws


def main():
    import torch

    import shs_gpu
    out = sys.argv[1] if len(sys.argv) > 1 else "-"
    trace = len(sys.argv) > 2 and sys.argv[2] == "trace"
    ctx = shs_gpu.Context(0)
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    ctx.set_stream(stream.cuda_stream)

    def one(k, ev=None):
        soft, pcf, draws = frames_of(k)
        ctx.rt_render_shadow(SM, soft.light_vp, draws, ref_tile=(TILE, TILE))
        if ev:
            ev[0].record(stream)
        ctx.rt_render(soft, draws)
        if ev:
            ev[1].record(stream)
        ctx.rt_render(pcf, draws)
        if ev:
            ev[2].record(stream)

    # the first soft frame builds the rotation table; a later one finds it
    soft, pcf, draws = frames_of(0)
    ctx.rt_render_shadow(SM, soft.light_vp, draws, ref_tile=(TILE, TILE))
    ctx.rt_render(pcf, draws)
    ctx.synchronize()
    t = time.perf_counter()
    ctx.rt_render(soft, draws)
    ctx.synchronize()
    first_ms = (time.perf_counter() - t) * 1e3
    t = time.perf_counter()
    ctx.rt_render(soft, draws)
    ctx.synchronize()
    later_ms = (time.perf_counter() - t) * 1e3

    for k in range(RAMP + WARM):
        one(k)
    ctx.synchronize()
    if trace:
        for k in range(FRAMES):
            one(k)
        ctx.synchronize()
        return
    evs = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(FRAMES)]
    for k in range(FRAMES):
        one(k, evs[k])
    ctx.synchronize()
    ts = [e[0].elapsed_time(e[1]) * 1e3 for e in evs]
    th = [e[1].elapsed_time(e[2]) * 1e3 for e in evs]
    st = ctx.rt_stats()
    shaded = int((ctx.rt_resolve_ids() >= 0).sum())
    lines = [f"exp_canvas_rt_soft: {W}x{H} tile {TILE}, map {SM}^2, {st['input_tris']} triangles ({st}), {shaded} shaded pixels, "
             f"{FRAMES} frames after {RAMP}+{WARM}"]
    for name, t_ in (("PASS1 soft (k_rt_setup<0> + k_rt_raster<0, 1>, PCSS 12 + 24 taps)", ts),
                     ("PASS1 hard (k_rt_setup<0> + k_rt_raster<0, 0>, 2x2 PCF)", th)):
        lines.append(f"  {name}: median {statistics.median(t_):.1f} us, mean {statistics.fmean(t_):.1f} us, min {min(t_):.1f}, max {max(t_):.1f}")
    ms, mh = statistics.median(ts), statistics.median(th)
    lines.append(f"  soft over hard: +{ms - mh:.1f} us per frame ({ms / mh:.2f}x), {1e3 * (ms - mh) / max(shaded, 1):.2f} ns per shaded pixel")
    lines.append(f"  rotation table: {W * H * 16} bytes; the first soft frame took {first_ms:.2f} ms on the host (build, upload, render), "
                 f"the next {later_ms:.2f} ms")
    text = "\n".join(lines)
    print(text)
    if out != "-":
        with open(os.path.join(ROOT, out) if not os.path.isabs(out) else out, "a") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
