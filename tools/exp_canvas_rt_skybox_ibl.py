"""The sky-lit camera pass (shs_rt_render_skybox_ibl, shading 4: PASS1 of hello_ibl_skybox.cpp) on that demo's own frame
(GPU box): 1200x900 (its CANVAS size, :43-44), tile jobs of 160, a 2048x2048 shadow map (its SHADOW_MAP_SIZE), its three
knob sets, and the scene of tools/exp_canvas_rt.py (the floor, a textured monkey standing in for the car, the monkey).

  python tools/exp_canvas_rt_skybox_ibl.py profiles/canvas_rt_skybox_ibl.txt        # appends its lines to the file
  python tools/exp_canvas_rt_skybox_ibl.py profiles/canvas_rt_skybox_ibl.txt hard   # the shading-0 passes alone: nothing
                                                                                    # newer than shs_rt_set_sky is called,
                                                                                    # so a checkout without shading 4 runs it
  python tools/exp_canvas_rt_skybox_ibl.py - trace                                  # FRAMES frames without events, for a
                                                                                    # `rocprofv3 --kernel-trace --stats -- python ...` run

One context on one stream.  After a clock ramp (RAMP frames) and WARM warm-up frames, FRAMES frames of PASS0 and then, under
no sky, the analytic sky and a 512x512-per-face cubemap sky (seeded random texels) in turn: the shading-4 PASS1 and the
shading-0 PASS1 (shs_rt_render: the same raster, the shader without the two sky samples) over the same map, a device event
before each camera pass and one after the last.  shs_rt_set_sky does no device work, so rebinding between the events
costs nothing on the stream.  With a sky bound the background pass follows both camera passes alike: the difference of
the two is the shader's."""
import dataclasses
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "leisure-software-renderer_amd"), ROOT, os.path.join(ROOT, "tools")]
import exp_canvas_rt as hard  # noqa: E402

FRAMES, WARM, RAMP = hard.FRAMES, hard.WARM, hard.RAMP
W, H, TILE, SM = 1200, 900, 160, 2048
FACE = 512
SKIES = ("none", "analytic", "cubemap")


def frames_of(k):
    frame, draws = hard.demo(0.2 * (k + 1), 0.2 * k)
    frame = dataclasses.replace(frame, width=W, height=H, ref_tile=(TILE, TILE))   # (the same 4:3 projection)
    return dataclasses.replace(frame, shading=4), frame, draws


def summary(t_):
    q = statistics.quantiles(t_, n=4)
    return f"median {statistics.median(t_):.1f} us, mean {statistics.fmean(t_):.1f} us, quartiles {q[0]:.1f} .. {q[2]:.1f}, min {min(t_):.1f}, max {max(t_):.1f}"


def main():
    import numpy as np
    import torch

    import shs_gpu
    out = sys.argv[1] if len(sys.argv) > 1 else "-"
    mode = sys.argv[2] if len(sys.argv) > 2 else "both"
    only_hard = mode == "hard"
    ctx = shs_gpu.Context(0)
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    ctx.set_stream(stream.cuda_stream)
    rng = np.random.default_rng(1)
    faces = tuple(ctx.upload_texture(hard.Texture(rng.integers(0, 256, (FACE, FACE, 4), dtype=np.uint8))) for _ in range(6))
    cam = dict(cam_forward=(0.0, 0.0, 1.0), cam_right=(1.0, 0.0, 0.0), cam_up=(0.0, 1.0, 0.0), fov_degrees=60.0)
    skies = {"none": None, "analytic": shs_gpu.RtSky(model=1, encode=1, **cam),
             "cubemap": shs_gpu.RtSky(model=2, encode=1, intensity=1.0, face_tex=faces, **cam)}
    if not only_hard:
        # hello_ibl_skybox.cpp:1299-1302 (floor), :1362-1365 (car), :1414-1417 (monkey)
        knobs = [shs_gpu.RtSkyboxIblDraw(0.30, 0.22, 0.04, 0.10), shs_gpu.RtSkyboxIblDraw(0.28, 0.38, 0.04, 0.60),
                 shs_gpu.RtSkyboxIblDraw(0.30, 0.32, 0.04, 0.35)]

    def one(k, ev=None):
        ibl, pcf, draws = frames_of(k)
        ctx.rt_render_shadow(SM, ibl.light_vp, draws, ref_tile=(TILE, TILE))
        for i, name in enumerate(SKIES):
            ctx.rt_set_sky(skies[name])
            if ev:
                ev[3 * i].record(stream)
            if not only_hard:
                ctx.rt_render_skybox_ibl(ibl, draws, knobs)
            if ev:
                ev[3 * i + 1].record(stream)
            ctx.rt_render(pcf, draws)
            if ev:
                ev[3 * i + 2].record(stream)

    for k in range(RAMP + WARM):
        one(k)
    ctx.synchronize()
    if mode == "trace":
        for k in range(FRAMES):
            one(k)
        ctx.synchronize()
        return
    evs = [[torch.cuda.Event(enable_timing=True) for _ in range(9)] for _ in range(FRAMES)]
    for k in range(FRAMES):
        one(k, evs[k])
    ctx.synchronize()
    st = ctx.rt_stats()
    shaded = int((ctx.rt_resolve_ids() >= 0).sum())
    lines = [f"exp_canvas_rt_skybox_ibl ({mode}): {W}x{H} tile {TILE}, map {SM}^2, cubemap {FACE}^2 per face, {st['input_tris']} triangles "
             f"({st}), {shaded} shaded pixels, {FRAMES} frames after {RAMP}+{WARM}"]
    for i, name in enumerate(SKIES):
        t4 = [e[3 * i].elapsed_time(e[3 * i + 1]) * 1e3 for e in evs]
        t0 = [e[3 * i + 1].elapsed_time(e[3 * i + 2]) * 1e3 for e in evs]
        if not only_hard:
            lines.append(f"  sky {name}: PASS1 shading 4 (k_rt_setup<0> + k_rt_raster<0, {4 + i}>): {summary(t4)}")
        lines.append(f"  sky {name}: PASS1 shading 0 (k_rt_setup<0> + k_rt_raster<0, 0>): {summary(t0)}")
        if not only_hard:
            m4, m0 = statistics.median(t4), statistics.median(t0)
            lines.append(f"  sky {name}: shading 4 over shading 0: {m4 - m0:+.1f} us per frame ({m4 / m0:.3f}x), "
                         f"{1e3 * (m4 - m0) / max(shaded, 1):.3f} ns per shaded pixel")
    text = "\n".join(lines)
    print(text)
    if out != "-":
        with open(os.path.join(ROOT, out) if not os.path.isabs(out) else out, "a") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
