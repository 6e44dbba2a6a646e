"""The Canvas render-target raster on hello_shadow_mapping.cpp's own frame (GPU box): 800x600, tile jobs of 80,
a 2048x2048 shadow map, FloorPlane(55, 140) with 48x48 cells, the monkey at the demo's transform and a second,
textured monkey standing in for the car (the Subaru asset is not in the repository), the light and camera of
main() and :1305-1317 (paths: the reference's cpp-folders/src/hello-render-target/).

  python tools/exp_canvas_rt.py profiles/canvas_rt.txt     # appends its lines to the file
  python tools/exp_canvas_rt.py - trace                    # FRAMES frames without events, for a
                                                           # `rocprofv3 --kernel-trace --stats -- python ...` run

After a clock ramp (RAMP frames) and WARM warm-up frames it times FRAMES frames with device events on the
context stream, one event before PASS0, one between the passes and one after PASS1, and reports each pass's
median and mean.  The algorithmic bytes of a pass -- every input read once, every record and plane written and
read once -- over its median time are given as a share of the HBM roofline (8.0 TB/s peak); the raster walks
its records many more times than once (per tile), out of L2, so the share says how far the pass is from a
bandwidth bound, not what it moves."""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "leisure-software-renderer_amd"), ROOT]
FRAMES, WARM, RAMP = int(os.environ.get("RT_FRAMES", 200)), int(os.environ.get("RT_WARM", 20)), int(os.environ.get("RT_RAMP", 40))
W, H, TILE, SM = 800, 600, 80, 2048
HBM_PEAK = 8.0e12


class Texture:
    def __init__(self, rgba):
        self.rgba = rgba


def floor_plane(half, forward, grid=48):
    import numpy as np
    from shs_gpu import scene
    xs = np.linspace(-half, half, grid + 1, dtype=np.float32)
    zs = np.linspace(0.0, forward, grid + 1, dtype=np.float32)
    tris, uvs = [], []
    for iz in range(grid):
        for ix in range(grid):
            p00, p10 = (xs[ix], 0, zs[iz]), (xs[ix + 1], 0, zs[iz])
            p11, p01 = (xs[ix + 1], 0, zs[iz + 1]), (xs[ix], 0, zs[iz + 1])
            tris += [np.concatenate([p00, p10, p11]), np.concatenate([p00, p11, p01])]
            uvs += [[0, 0, 1, 0, 1, 1], [0, 0, 1, 1, 0, 1]]
    pos = np.array(tris, np.float32)
    return scene.Mesh(pos, np.tile(np.array([0, 1, 0] * 3, np.float32), (len(tris), 1)), np.array(uvs, np.float32))


def demo(angle, prev_angle):
    import numpy as np
    import shs_gpu
    from shs_gpu import lib_path, scene
    from shs_gpu import _abi
    import ctypes
    cam = (0.0, 10.0, -42.0)
    view, proj = scene.camera(cam, 0.0, 0.0)
    vp = scene.mat_mul(proj, view)
    d = np.array([0.4668, -0.3487, 0.8127])
    d = d / np.linalg.norm(d)
    center = np.array([0.0, 6.0, 45.0])
    light_view = lib_path.look_at_lh(tuple(center - d * 80.0), tuple(center))
    ortho = np.zeros(16, np.float32)
    assert _abi.lib().shs_ortho_lh_zo(-85.0, 85.0, -55.0, 95.0, 0.1, 240.0, ortho.ctypes.data_as(ctypes.POINTER(ctypes.c_float))) == 0
    light_vp = scene.mat_mul(ortho, light_view)
    eye = np.eye(4, dtype=np.float32).reshape(16)
    rng = np.random.default_rng(0)
    tex = demo.tex = getattr(demo, "tex", None) or Texture(rng.integers(0, 256, (256, 256, 4), dtype=np.uint8))
    floor = demo.floor = getattr(demo, "floor", None) or floor_plane(55.0, 140.0)

    def draw(mesh, model, prev, color, t=None):
        return shs_gpu.RtDraw(mesh, model, scene.mat_mul(vp, model), scene.mat_mul(vp, prev), color, t)
    m_car = scene.model_trs((-6.0, 4.0, 26.0), -angle, (4.0, 4.0, 4.0))
    p_car = scene.model_trs((-6.0, 4.0, 26.0), -prev_angle, (4.0, 4.0, 4.0))
    m_mk = scene.model_trs((-6.0, 12.2, 26.0), 3.0 * angle, (1.65, 1.65, 1.65))
    p_mk = scene.model_trs((-6.0, 12.2, 26.0), 3.0 * prev_angle, (1.65, 1.65, 1.65))
    draws = [draw(floor, eye, eye, (120, 122, 128, 255)), draw(scene.monkey(), m_car, p_car, (200, 200, 200, 255), tex),
             draw(scene.monkey(), m_mk, p_mk, (180, 150, 95, 255))]
    frame = shs_gpu.RtFrame(W, H, view, light_vp, tuple(d), cam, ref_tile=(TILE, TILE))
    return frame, draws


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
        frame, draws = demo(0.2 * (k + 1), 0.2 * k)
        if ev:
            ev[0].record(stream)
        ctx.rt_render_shadow(SM, frame.light_vp, draws, ref_tile=(TILE, TILE))
        if ev:
            ev[1].record(stream)
        ctx.rt_render(frame, draws)
        if ev:
            ev[2].record(stream)
        return draws
    for k in range(RAMP + WARM):
        draws = one(k)
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
    t0 = [e[0].elapsed_time(e[1]) * 1e3 for e in evs]
    t1 = [e[1].elapsed_time(e[2]) * 1e3 for e in evs]
    st = ctx.rt_stats()
    n = st["input_tris"]
    uv_tris = sum(d.mesh.positions.shape[0] for d in draws if d.mesh.uvs is not None)
    b0 = n * 36 + n * 96 * 2 + SM * SM * 4
    b1 = n * 72 + uv_tris * 24 + 2 * n * 96 * 2 + st["sub_tris"] * 192 * 2 + W * H * (4 + 4 + 8 + 4) + SM * SM * 4
    lines = [f"exp_canvas_rt: {W}x{H} tile {TILE}, map {SM}^2, {n} triangles ({st}), {FRAMES} frames after {RAMP}+{WARM}"]
    for name, t, b in (("PASS0 shadow (k_rt_setup<1> + k_rt_raster<1>)", t0, b0), ("PASS1 camera (k_rt_setup<0> + k_rt_raster<0>)", t1, b1)):
        med = statistics.median(t)
        lines.append(f"  {name}: median {med:.1f} us, mean {statistics.fmean(t):.1f} us, min {min(t):.1f}, max {max(t):.1f}; "
                     f"algorithmic {b / 1e6:.2f} MB -> {b / (med * 1e-6) / 1e9:.1f} GB/s = "
                     f"{100.0 * b / (med * 1e-6) / HBM_PEAK:.2f} % of the HBM roofline ({HBM_PEAK / 1e12:.1f} TB/s)")
    text = "\n".join(lines)
    print(text)
    if out != "-":
        with open(os.path.join(ROOT, out) if not os.path.isabs(out) else out, "a") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
