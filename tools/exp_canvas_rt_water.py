"""hello_water.cpp's camera pass (shs_rt_render_water, shading 5) on that demo's own frame (GPU box): 380x280 with tile jobs of
80 (its CANVAS size and TILE_SIZE, :41-47) or 1200x900 with tile jobs of 160 (the size the other render-target profiles
use), a 2048x2048 shadow map (its SHADOW_MAP_SIZE), a 56 x 56-quad water plane of 120 x 160 world units (WaterPlane :578-629)
over the scene of tools/exp_canvas_rt.py (the floor, a textured monkey standing in for the car, the monkey).

  python tools/exp_canvas_rt_water.py profiles/canvas_rt_water.txt both 380    # appends its lines to the file
  python tools/exp_canvas_rt_water.py profiles/canvas_rt_water.txt hard 1200   # the shading-0 pass alone: nothing newer than
                                                                               # shs_rt_render is called, so a checkout
                                                                               # without shading 5 runs it
  python tools/exp_canvas_rt_water.py - trace 1200                             # FRAMES frames without events, for a
                                                                               # `rocprofv3 --kernel-trace --stats -- python ...` run

One context on one stream.  After a clock ramp (RAMP frames) and WARM warm-up frames, FRAMES frames of: PASS0; the
reflection pass from the mirrored camera (shading 5, the objects alone) and shs_rt_keep_reflection; the shading-5 camera
pass over floor, water and objects; the shading-0 camera pass (shs_rt_render) over the same draws, the water plane drawn as
a plain object -- the same raster, the hard demo's shader on every pixel.  A device event before each and one after the last."""
import dataclasses
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "leisure-software-renderer_amd"), ROOT, os.path.join(ROOT, "tools")]
import exp_canvas_rt as hard  # noqa: E402

FRAMES, WARM, RAMP = hard.FRAMES, hard.WARM, hard.RAMP
SM = 2048
SIZES = {"380": (380, 280, 80), "1200": (1200, 900, 160)}
WATER_Y = 0.5
GRID = 56


def water_plane():
    """WaterPlane :578-629: GRID x GRID quads over x in [-60, 60], z in [-20, 140], the normal up"""
    import numpy as np
    xs, zs = np.linspace(-60.0, 60.0, GRID + 1), np.linspace(-20.0, 140.0, GRID + 1)
    tris = []
    for j in range(GRID):
        for i in range(GRID):
            a, b, c, d = (xs[i], WATER_Y, zs[j]), (xs[i + 1], WATER_Y, zs[j]), (xs[i + 1], WATER_Y, zs[j + 1]), (xs[i], WATER_Y, zs[j + 1])
            tris += [np.concatenate([a, c, b]), np.concatenate([a, d, c])]
    from shs_gpu import scene
    return scene.Mesh(np.array(tris, np.float32), np.tile(np.array([0, 1, 0] * 3, np.float32), (len(tris), 1)), None)


def frames_of(k, size):
    import numpy as np
    import shs_gpu
    from shs_gpu import scene
    w, h, tile = SIZES[size]
    frame, draws = hard.demo(0.2 * (k + 1), 0.2 * k)
    frame = dataclasses.replace(frame, width=w, height=h, ref_tile=(tile, tile))   # (the same 4:3 projection)
    proj = scene.camera(frame.camera_pos, 0.0, 0.0)[1]
    vp = scene.mat_mul(proj, frame.view)
    eye = np.eye(4, dtype=np.float32).reshape(16)
    plane = frames_of.plane = getattr(frames_of, "plane", None) or water_plane()
    water = shs_gpu.RtDraw(plane, eye, vp, vp, (10, 40, 60, 255), None)
    return frame, draws[:1] + [water] + draws[1:], proj


def summary(t_):
    q = statistics.quantiles(t_, n=4)
    return f"median {statistics.median(t_):.1f} us, mean {statistics.fmean(t_):.1f} us, quartiles {q[0]:.1f} .. {q[2]:.1f}, min {min(t_):.1f}, max {max(t_):.1f}"


def main():
    import numpy as np
    import torch

    import shs_gpu
    from shs_gpu import lib_path, scene
    out = sys.argv[1] if len(sys.argv) > 1 else "-"
    mode = sys.argv[2] if len(sys.argv) > 2 else "both"
    size = sys.argv[3] if len(sys.argv) > 3 else "380"
    only_hard = mode == "hard"
    w, h, tile = SIZES[size]
    ctx = shs_gpu.Context(0)
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    ctx.set_stream(stream.cuda_stream)

    def one(k, ev=None):
        frame, draws, proj = frames_of(k, size)
        ctx.rt_render_shadow(SM, frame.light_vp, draws, ref_tile=(tile, tile))
        if ev:
            ev[0].record(stream)
        if not only_hard:
            # compute_reflection_view_lh :1550-1563: the camera looks along +z, mirrored at y = WATER_Y
            cam = frame.camera_pos
            mpos = (cam[0], 2.0 * WATER_Y - cam[1], cam[2])
            rview = lib_path.look_at_lh(mpos, (mpos[0], mpos[1], mpos[2] + 1.0), (0.0, -1.0, 0.0))
            rvp = scene.mat_mul(proj, rview)
            objs = [dataclasses.replace(d, mvp=scene.mat_mul(rvp, d.model), prev_mvp=scene.mat_mul(rvp, d.model)) for d in draws[:1] + draws[2:]]
            refl = dataclasses.replace(frame, shading=5, view=rview, camera_pos=mpos)
            ctx.rt_render_water(refl, objs, [shs_gpu.RtWaterDraw(False)] * len(objs), shs_gpu.RtWater(None, 0.1 * k, False))
            ctx.rt_keep_reflection()
        if ev:
            ev[1].record(stream)
        if not only_hard:
            flags = [shs_gpu.RtWaterDraw(i == 1) for i in range(len(draws))]
            ctx.rt_render_water(dataclasses.replace(frame, shading=5), draws, flags, shs_gpu.RtWater(rvp, 0.1 * k, True))
        if ev:
            ev[2].record(stream)
        ctx.rt_render(frame, draws)
        if ev:
            ev[3].record(stream)
        return draws

    for k in range(RAMP + WARM):
        one(k)
    ctx.synchronize()
    if mode == "trace":
        for k in range(FRAMES):
            one(k)
        ctx.synchronize()
        return
    evs = [[torch.cuda.Event(enable_timing=True) for _ in range(4)] for _ in range(FRAMES)]
    for k in range(FRAMES):
        draws = one(k, evs[k])
    ctx.synchronize()
    st = ctx.rt_stats()
    ids = ctx.rt_resolve_ids()
    shaded = int((ids >= 0).sum())
    n0 = draws[0].mesh.positions.shape[0]
    n1 = draws[1].mesh.positions.shape[0]
    water_px = int(((ids // 2 >= n0) & (ids // 2 < n0 + n1) & (ids >= 0)).sum())
    lines = [f"exp_canvas_rt_water ({mode}): {w}x{h} tile {tile}, map {SM}^2, {st['input_tris']} triangles ({st}), {shaded} shaded pixels "
             f"of {w * h}, {water_px} of them water ({water_px / (w * h):.3f} of the frame), {FRAMES} frames after {RAMP}+{WARM}"]
    t_refl = [e[0].elapsed_time(e[1]) * 1e3 for e in evs]
    t5 = [e[1].elapsed_time(e[2]) * 1e3 for e in evs]
    t0 = [e[2].elapsed_time(e[3]) * 1e3 for e in evs]
    if not only_hard:
        lines.append(f"  reflection pass (shading 5, objects alone) + keep: {summary(t_refl)}")
        lines.append(f"  PASS1 shading 5 (k_rt_setup<0> + k_rt_raster<0, water>): {summary(t5)}")
    lines.append(f"  PASS1 shading 0 over the same draws (k_rt_setup<0> + k_rt_raster<0, 0>): {summary(t0)}")
    if not only_hard:
        m5, m0 = statistics.median(t5), statistics.median(t0)
        lines.append(f"  shading 5 over shading 0: {m5 - m0:+.1f} us per frame ({m5 / m0:.3f}x), {1e3 * (m5 - m0) / max(water_px, 1):.3f} ns per water pixel")
    text = "\n".join(lines)
    print(text)
    if out != "-":
        with open(os.path.join(ROOT, out) if not os.path.isabs(out) else out, "a") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
