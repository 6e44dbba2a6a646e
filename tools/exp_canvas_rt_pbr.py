"""The GGX + IBL camera pass on hello_pbr.cpp's own frame (GPU box): 1200x900, tile jobs of 160, a 2048x2048 shadow
map, irradiance 16^2 and a prefiltered-specular chain of base 256 with 6 mips (seeded random floats), the scene of
tools/exp_canvas_rt.py (FloorPlane(55, 140) with 48x48 cells, the monkey at the demo's transform and a second,
textured monkey standing in for the car) under the demo's three materials and constants.

  python tools/exp_canvas_rt_pbr.py profiles/canvas_rt_pbr.txt   # appends its lines to the file
  python tools/exp_canvas_rt_pbr.py - trace                      # FRAMES frames without events, for a
                                                                 # `rocprofv3 --kernel-trace --stats -- python ...` run

After a clock ramp (RAMP frames) and WARM warm-up frames it times FRAMES frames with device events on the context
stream.  Each frame is PASS0, then the PBR PASS1 (shs_rt_render_pbr), then the PBR PASS1 without an IBL's levels
bound (the same kernel, no gathers), then the hard PCF PASS1 (shading 0) of the same scene and tile size over the
same map, one event before each and one after the last: the camera passes are measured in the same run under the
same clocks.  The middle pass separates the 12 IBL gathers from the shader's arithmetic."""
import dataclasses
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "leisure-software-renderer_amd"), ROOT, os.path.join(ROOT, "tools")]
import exp_canvas_rt as hard  # noqa: E402

FRAMES, WARM, RAMP = hard.FRAMES, hard.WARM, hard.RAMP
W, H, TILE, SM = 1200, 900, 160, 2048
IRR, SPEC_BASE, MIPS = 16, 256, 6


def make_ibl():
    import numpy as np
    rng = np.random.default_rng(0)
    irr = rng.uniform(0.0, 4.0, (6, IRR, IRR, 3)).astype(np.float32)
    spec = [rng.uniform(0.0, 4.0, (6, SPEC_BASE >> m, SPEC_BASE >> m, 3)).astype(np.float32) for m in range(MIPS)]
    return irr, spec


def frames_of(k):
    import numpy as np
    import shs_gpu
    frame, draws = hard.demo(0.2 * (k + 1), 0.2 * k)
    frame = dataclasses.replace(frame, width=W, height=H, ref_tile=(TILE, TILE))   # (the same 4:3 projection)

    def n3(model):   # transpose(inverse(mat3(model))), column-major
        return np.linalg.inv(np.asarray(model, np.float64).reshape(4, 4).T[:3, :3]).astype(np.float32).reshape(9)
    # hello_pbr.cpp:1493-1504 (floor), :1568-1579 (car), :1630-1641 (monkey)
    mats = [shs_gpu.RtPbrDraw(None, 0.0, 0.70, 1.0, 1.30, 0.60, 0.20), shs_gpu.RtPbrDraw(n3(draws[1].model), 0.0, 0.22, 1.0, 1.50, 1.00, 1.20),
            shs_gpu.RtPbrDraw(n3(draws[2].model), 0.95, 0.20, 1.0, 1.00, 1.80, 1.00)]
    draws[2] = dataclasses.replace(draws[2], base_color=(240, 195, 75, 255))
    return dataclasses.replace(frame, shading=2), frame, draws, mats


def main():
    import torch

    import shs_gpu
    out = sys.argv[1] if len(sys.argv) > 1 else "-"
    trace = len(sys.argv) > 2 and sys.argv[2] == "trace"
    ctx = shs_gpu.Context(0)
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    ctx.set_stream(stream.cuda_stream)
    ibl = make_ibl()
    ctx.rt_set_ibl(*ibl)
    # a second context for the pass without an IBL: shs_rt_set_ibl is synchronous, so switching inside a frame would
    # put an upload and two synchronisations between the events
    bare = shs_gpu.Context(0)
    bare.set_stream(stream.cuda_stream)

    def one(k, ev=None):
        pbr, pcf, draws, mats = frames_of(k)
        ctx.rt_render_shadow(SM, pbr.light_vp, draws, ref_tile=(TILE, TILE))
        bare.rt_render_shadow(SM, pbr.light_vp, draws, ref_tile=(TILE, TILE))
        if ev:
            ev[0].record(stream)
        ctx.rt_render_pbr(pbr, draws, mats)
        if ev:
            ev[1].record(stream)
        bare.rt_render_pbr(pbr, draws, mats)
        if ev:
            ev[2].record(stream)
        ctx.rt_render(pcf, draws)
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
    tp = [e[0].elapsed_time(e[1]) * 1e3 for e in evs]
    tb = [e[1].elapsed_time(e[2]) * 1e3 for e in evs]
    th = [e[2].elapsed_time(e[3]) * 1e3 for e in evs]
    st = ctx.rt_stats()
    shaded = int((ctx.rt_resolve_ids() >= 0).sum())
    texels = 6 * (IRR * IRR + sum((SPEC_BASE >> m) ** 2 for m in range(MIPS)))
    lines = [f"exp_canvas_rt_pbr: {W}x{H} tile {TILE}, map {SM}^2, irradiance {IRR}^2, specular {SPEC_BASE} x {MIPS} mips "
             f"({texels} texels, {16 * (texels + 17)} bytes), {st['input_tris']} triangles ({st}), {shaded} shaded pixels, "
             f"{FRAMES} frames after {RAMP}+{WARM}"]
    for name, t_ in (("PASS1 pbr  (k_rt_setup<0> + k_rt_raster<0, 2>, GGX + 12 IBL gathers)", tp),
                     ("PASS1 pbr without an IBL (the same kernels, no gathers)", tb),
                     ("PASS1 hard (k_rt_setup<0> + k_rt_raster<0, 0>, 2x2 PCF)", th)):
        lines.append(f"  {name}: median {statistics.median(t_):.1f} us, mean {statistics.fmean(t_):.1f} us, min {min(t_):.1f}, max {max(t_):.1f}")
    mp, mb, mh = statistics.median(tp), statistics.median(tb), statistics.median(th)
    lines.append(f"  pbr over hard: {mp - mh:+.1f} us per frame ({mp / mh:.2f}x), {1e3 * (mp - mh) / max(shaded, 1):.2f} ns per shaded pixel; "
                 f"of it the IBL gathers {mp - mb:+.1f} us, the rest of the shader {mb - mh:+.1f} us")
    text = "\n".join(lines)
    print(text)
    if out != "-":
        with open(os.path.join(ROOT, out) if not os.path.isabs(out) else out, "a") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
