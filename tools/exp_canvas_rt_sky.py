"""The background pass behind the GGX + IBL camera pass on hello_pbr.cpp's own frame (GPU box): the frame of
tools/exp_canvas_rt_pbr.py (1200x900, tile jobs of 160, a 2048x2048 shadow map, its IBL, scene, materials and constants)
with no sky, with the demo's AnalyticSky (its default sun, SKY_EXPOSURE 1.85, the Reinhard encode) and with a CubeMapSky of
six 512x512 faces of seeded random bytes.

  python tools/exp_canvas_rt_sky.py profiles/canvas_rt_sky.txt   # appends its lines to the file
  python tools/exp_canvas_rt_sky.py - trace                      # FRAMES frames without events, for a
                                                                 # `rocprofv3 --kernel-trace --stats -- python ...` run

Three contexts on one stream, one per sky (shs_rt_set_sky is per context; a context each keeps the binding out of the
timed window).  After a clock ramp (RAMP frames) and WARM warm-up frames it times FRAMES frames with device events: each
frame is the three contexts' PASS0, then the three PBR PASS1 (shs_rt_render_pbr) one after another -- no sky, analytic,
cubemap, the order rotating from frame to frame -- with one event before each and one after the last, so the three are
measured in the same run under the same clocks.  k_rt_sky's own time is a with-sky pass minus the no-sky pass of the
same frame (the trace run gives it per kernel)."""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "leisure-software-renderer_amd"), ROOT, os.path.join(ROOT, "tools")]
import exp_canvas_rt_pbr as pbr  # noqa: E402

FRAMES, WARM, RAMP = pbr.FRAMES, pbr.WARM, pbr.RAMP
W, H, TILE, SM = pbr.W, pbr.H, pbr.TILE, pbr.SM
FACE = 512
NAMES = ("no sky", "analytic sky", f"cubemap sky {FACE}^2")


def skies(view):
    import numpy as np
    import shs_gpu
    m = np.asarray(view, np.float32).reshape(4, 4)   # lookAtLH's rows: right, up, forward
    cam = dict(cam_right=tuple(float(v) for v in m[:3, 0]), cam_up=tuple(float(v) for v in m[:3, 1]),
               cam_forward=tuple(float(v) for v in m[:3, 2]), fov_degrees=60.0)
    rng = np.random.default_rng(1)
    faces = tuple(pbr.hard.Texture(rng.integers(0, 256, (FACE, FACE, 4), dtype=np.uint8)) for _ in range(6))
    return [None, shs_gpu.RtSky(**cam), shs_gpu.RtSky(model=2, face_tex=faces, **cam)]


def main():
    import torch

    import shs_gpu
    out = sys.argv[1] if len(sys.argv) > 1 else "-"
    trace = len(sys.argv) > 2 and sys.argv[2] == "trace"
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    ibl = pbr.make_ibl()
    frame0 = pbr.frames_of(0)[0]
    ctxs = []
    for sky in skies(frame0.view):
        c = shs_gpu.Context(0)
        c.set_stream(stream.cuda_stream)
        c.rt_set_ibl(*ibl)
        c.rt_set_sky(sky)
        ctxs.append(c)

    def one(k, ev=None):
        frame, _, draws, mats = pbr.frames_of(k)
        for c in ctxs:
            c.rt_render_shadow(SM, frame.light_vp, draws, ref_tile=(TILE, TILE))
        order = [(k + j) % 3 for j in range(3)]
        for j, i in enumerate(order):
            if ev:
                ev[j].record(stream)
            ctxs[i].rt_render_pbr(frame, draws, mats)
        if ev:
            ev[3].record(stream)
        return order

    for k in range(RAMP + WARM):
        one(k)
    ctxs[0].synchronize()
    if trace:
        for k in range(FRAMES):
            one(k)
        ctxs[0].synchronize()
        return
    evs = [[torch.cuda.Event(enable_timing=True) for _ in range(4)] for _ in range(FRAMES)]
    orders = [one(k, evs[k]) for k in range(FRAMES)]
    ctxs[0].synchronize()
    t = [[0.0] * FRAMES for _ in range(3)]
    for k, (e, order) in enumerate(zip(evs, orders)):
        for j, i in enumerate(order):
            t[i][k] = e[j].elapsed_time(e[j + 1]) * 1e3
    ids = ctxs[1].rt_resolve_ids()
    sky_px = int((ids < 0).sum())
    st = ctxs[1].rt_stats()
    lines = [f"exp_canvas_rt_sky: {W}x{H} tile {TILE}, map {SM}^2, {st['input_tris']} triangles, {sky_px} sky pixels of {W * H}, "
             f"{FRAMES} frames after {RAMP}+{WARM}"]
    for name, t_ in zip(NAMES, t):
        lines.append(f"  PASS1 pbr, {name}: median {statistics.median(t_):.1f} us, mean {statistics.fmean(t_):.1f} us, "
                     f"min {min(t_):.1f}, max {max(t_):.1f}")
    spread = max(t[0]) - min(t[0])
    for i in (1, 2):
        d = [a - b for a, b in zip(t[i], t[0])]
        md = statistics.median(d)
        lines.append(f"  k_rt_sky, {NAMES[i]} (the pass minus the same frame's no-sky pass): median {md:+.1f} us, min {min(d):+.1f}, "
                     f"max {max(d):+.1f}; {1e3 * md / max(sky_px, 1):.3f} ns per sky pixel; the no-sky pass's min-max spread is {spread:.1f} us")
    text = "\n".join(lines)
    print(text)
    if out != "-":
        with open(os.path.join(ROOT, out) if not os.path.isabs(out) else out, "a") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
