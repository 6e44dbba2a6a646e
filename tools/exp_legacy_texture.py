"""What the texture-mapping pipeline (SHADING_TEXTURED) costs on the C2 scene (GPU box): bench.py's C2 step --
one shs_render_legacy_batch of FRAMES camera poses of Suzanne at 1920x1080 -- with the draw's model swapped
for the textured one (the monkey's own UVs, a 256x256 texture), against Blinn-Phong on the same commit.

  python tools/exp_legacy_texture.py profiles/legacy_texture.txt      # appends its lines to the file

tools/exp_legacy_shaders.py's pattern: one process, one context, the rows interleaved over ROUNDS rounds (a
round times RUNS steps of every row after WARM warm-up steps, one event pair per step on the context
stream); Blinn-Phong is timed twice per round, first and last, and the difference of its two medians is the
noise.  A textured batch runs the third compilation (RF_TEX_MODEL), whose every pair test reads a staged side
entry and whose poses share no varyings; the row 'blinn_phong (tex kernels)' -- a Blinn-Phong draw beside a
textured draw of one hidden triangle -- separates that compilation's cost from the model's own arithmetic
('blinn_phong + speck' is its control), and 'textured, no texture' leaves the sampler out."""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "leisure-software-renderer_amd"), ROOT]
FRAMES = int(os.environ.get("LS_FRAMES", 128))
ROUNDS, RUNS, WARM = int(os.environ.get("LS_ROUNDS", 5)), int(os.environ.get("LS_RUNS", 30)), int(os.environ.get("LS_WARM", 5))


class Texture:
    def __init__(self, rgba):
        self.rgba = rgba


def main():
    import copy

    import numpy as np
    import torch

    import bench
    import shs_gpu
    from shs_gpu import scene

    frame, sets = bench.batch_poses("c2", FRAMES)
    fds = sets[0]
    assert scene.monkey().uvs is not None
    rng = np.random.default_rng(0)
    tex = Texture(rng.integers(0, 256, (256, 256, 4), dtype=np.uint8))
    speck = scene.Mesh(np.array([[0, 0, 0, 1e-3, 0, 0, 0, 1e-3, 0]], np.float32), np.array([[0, 0, 1] * 3], np.float32))
    ctx = shs_gpu.Context(0)
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    ctx.set_stream(stream.cuda_stream)

    def batch(model, albedo=None, extra=None):
        out = []
        for draws in fds:
            d = copy.copy(draws[0])
            d.shading, d.albedo_tex = model, albedo
            row = [d]
            if extra is not None:   # a second draw: one tiny triangle hidden inside Suzanne
                e = copy.copy(draws[0])
                e.mesh, e.shading = speck, extra
                e.albedo_tex = 0 if extra == shs_gpu.SHADING_TEXTURED else None   # (0: the textured call, no texture)
                row.append(e)
            out.append(row)
        return ctx.prepare_batch(frame, out)

    T = shs_gpu.SHADING_TEXTURED
    rows = [("blinn_phong", batch(3)), ("textured", batch(T, tex)), ("textured, no texture", batch(T, 0)),
            ("blinn_phong + speck", batch(3, None, 3)), ("blinn_phong (tex kernels)", batch(3, None, T)),
            ("blinn_phong again", batch(3))]
    covered = None
    med = {k: [] for k, _ in rows}
    for _ in range(ROUNDS):
        for name, prepared in rows:
            for _ in range(WARM):
                ctx.render_batch_prepared(prepared)
            torch.cuda.synchronize()
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(RUNS)]
            for a, b in ev:
                a.record()
                ctx.render_batch_prepared(prepared)
                b.record()
            torch.cuda.synchronize()
            med[name].append(statistics.median(a.elapsed_time(b) * 1e3 for a, b in ev))
            if covered is None:
                covered = ctx.stats()["covered_pixels"]
    ctx.close()
    lines = [f"textured model on C2: one batch of {FRAMES} poses at {frame.width}x{frame.height} per step "
             f"({covered} covered pixels per batch, {100.0 * covered / (FRAMES * frame.width * frame.height):.1f} % of the pixels), "
             f"us per step: median over {ROUNDS} interleaved rounds of the medians of {RUNS} steps (min-max of the rounds)"]
    base = statistics.median(med["blinn_phong"])
    for name, _ in rows:
        v = med[name]
        m = statistics.median(v)
        lines.append(f"  {name:27s} {m:8.1f} ({min(v):.1f}-{max(v):.1f})  {m - base:+7.1f} us  {100.0 * (m - base) / base:+5.1f} %")
    print("\n".join(lines), flush=True)
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
