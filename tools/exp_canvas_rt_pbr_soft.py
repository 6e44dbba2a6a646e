"""PBR under PCSS (shs_rt_render_pbr_soft, shading 3: PASS1 of hello_pbr_light_shafts.cpp) on that demo's frame (GPU box):
800x600 (its WINDOW / CANVAS size, :108-111), tile jobs of 160, a 1024x1024 shadow map (its SHADOW_MAP_SIZE), the demo's
PCSS and PBR constants (the contexts' defaults) and three materials; the scene, camera, light and IBL are
tools/exp_canvas_rt_pbr.py's.

  python tools/exp_canvas_rt_pbr_soft.py profiles/canvas_rt_pbr_soft.txt   # appends its lines to the file
  python tools/exp_canvas_rt_pbr_soft.py - trace                           # FRAMES frames without events, for a
                                                                           # `rocprofv3 --kernel-trace --stats -- python ...` run

One context on one stream.  The first shading-3 frame of a size builds the per-pixel rotation table on the host and
uploads it: that call is timed on the host clock against the second frame's.  Then, after a clock ramp (RAMP frames) and
WARM warm-up frames, FRAMES frames of PASS0, the shading-3 PASS1 and the shading-2 PASS1 (shs_rt_render_pbr: the same
shader under the 2x2 PCF, with the minimum ambient) over the same map, a device event before each camera pass and one
after the last, so the two are measured in the same run under the same clocks."""
import dataclasses
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "leisure-software-renderer_amd"), ROOT, os.path.join(ROOT, "tools")]
import exp_canvas_rt_pbr as pbr  # noqa: E402

FRAMES, WARM, RAMP = pbr.FRAMES, pbr.WARM, pbr.RAMP
W, H, TILE, SM = 800, 600, 160, 1024


def frames_of(k):
    hard2, _, draws, mats = pbr.frames_of(k)
    hard2 = dataclasses.replace(hard2, width=W, height=H, ref_tile=(TILE, TILE))   # (the same 4:3 projection)
    return dataclasses.replace(hard2, shading=3), hard2, draws, mats


def main():
    import torch

    import shs_gpu
    out = sys.argv[1] if len(sys.argv) > 1 else "-"
    trace = len(sys.argv) > 2 and sys.argv[2] == "trace"
    ctx = shs_gpu.Context(0)
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    ctx.set_stream(stream.cuda_stream)
    ctx.rt_set_ibl(*pbr.make_ibl())

    def one(k, ev=None):
        soft, pcf, draws, mats = frames_of(k)
        ctx.rt_render_shadow(SM, soft.light_vp, draws, ref_tile=(TILE, TILE))
        if ev:
            ev[0].record(stream)
        ctx.rt_render_pbr_soft(soft, draws, mats)
        if ev:
            ev[1].record(stream)
        ctx.rt_render_pbr(pcf, draws, mats)
        if ev:
            ev[2].record(stream)

    # the rotation table's first-frame cost: the shading-2 pass first, so that every other buffer of the size exists
    soft, pcf, draws, mats = frames_of(0)
    ctx.rt_render_shadow(SM, soft.light_vp, draws, ref_tile=(TILE, TILE))
    ctx.rt_render_pbr(pcf, draws, mats)
    ctx.synchronize()
    first = []
    for _ in range(2):
        t0 = time.perf_counter()
        ctx.rt_render_pbr_soft(soft, draws, mats)
        ctx.synchronize()
        first.append((time.perf_counter() - t0) * 1e3)
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
    tp = [e[1].elapsed_time(e[2]) * 1e3 for e in evs]
    st = ctx.rt_stats()
    shaded = int((ctx.rt_resolve_ids() >= 0).sum())
    last, _, draws, mats = frames_of(FRAMES - 1)
    ctx.rt_render_pbr_soft(dataclasses.replace(last, prequant=True), draws, mats)
    fac = ctx.rt_resolve_prequant()[..., 3]
    lines = [f"exp_canvas_rt_pbr_soft: {W}x{H} tile {TILE}, map {SM}^2, {st['input_tris']} triangles ({st}), {shaded} shaded pixels, "
             f"{FRAMES} frames after {RAMP}+{WARM}"]
    lines.append(f"  PCSS factors of the last frame: {int(((fac == 0) & (ctx.rt_resolve_ids() >= 0)).sum())} shaded pixels at 0, "
                 f"{int(((fac > 0) & (fac < 1)).sum())} between 0 and 1")
    lines.append(f"  rotation table ({W * H * 16} bytes): first shading-3 call of the size {first[0]:.2f} ms on the host clock "
                 f"(table build, upload, the pass), the second {first[1]:.2f} ms")
    for name, t_ in (("PASS1 shading 3 (k_rt_setup<0> + k_rt_raster<0, 3>, GGX + IBL under PCSS)", ts),
                     ("PASS1 shading 2 (k_rt_setup<0> + k_rt_raster<0, 2>, GGX + IBL under the 2x2 PCF)", tp)):
        lines.append(f"  {name}: median {statistics.median(t_):.1f} us, mean {statistics.fmean(t_):.1f} us, min {min(t_):.1f}, max {max(t_):.1f}")
    ms, mp = statistics.median(ts), statistics.median(tp)
    lines.append(f"  shading 3 over shading 2: {ms - mp:+.1f} us per frame ({ms / mp:.3f}x), {1e3 * (ms - mp) / max(shaded, 1):.2f} ns per shaded pixel")
    text = "\n".join(lines)
    print(text)
    if out != "-":
        with open(os.path.join(ROOT, out) if not os.path.isabs(out) else out, "a") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
