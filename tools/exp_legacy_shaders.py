"""What the Toon, Gooch, Oren-Nayar, normal- and depth-visualiser shading models cost on the C2 scene (GPU box):
bench.py's C2 step -- one shs_render_legacy_batch of FRAMES camera poses of Suzanne at 1920x1080 -- with the
draw's shading model swapped, against Blinn-Phong on the same commit.

  python tools/exp_legacy_shaders.py profiles/legacy_shaders.txt      # appends its lines to the file

One process, one context; the models are interleaved over ROUNDS rounds (a round times RUNS steps of every
model after WARM warm-up steps, one event pair per step on the context stream), so clock drift and the
machine's other tenants hit every model alike.  Blinn-Phong is timed twice per round, first and last: the
difference of its two medians is the noise a model's difference has to be read against.  A Blinn-Phong batch
runs the kernels without the new models' code, every other batch the compilation that has them
(RF_EXT_MODELS), so a new model's figure holds both that compilation's cost and its own arithmetic; the row
'blinn_phong (ext kernels)' separates the two: a Blinn-Phong draw beside a Toon draw of one hidden triangle
(and, as its control, 'blinn_phong + speck': beside a Blinn-Phong one)."""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "leisure-software-renderer_amd"), ROOT]
FRAMES = int(os.environ.get("LS_FRAMES", 128))
ROUNDS, RUNS, WARM = int(os.environ.get("LS_ROUNDS", 5)), int(os.environ.get("LS_RUNS", 30)), int(os.environ.get("LS_WARM", 5))


def main():
    import copy

    import numpy as np
    import torch

    import bench
    import shs_gpu
    from shs_gpu import scene

    frame, sets = bench.batch_poses("c2", FRAMES)
    fds = sets[0]
    names = {v: k for k, v in shs_gpu.SHADING_NAMES.items()}
    speck = scene.Mesh(np.array([[0, 0, 0, 1e-3, 0, 0, 0, 1e-3, 0]], np.float32), np.array([[0, 0, 1] * 3], np.float32))
    ctx = shs_gpu.Context(0)
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    ctx.set_stream(stream.cuda_stream)

    def batch(model, extra=None):
        out = []
        for draws in fds:
            d = copy.copy(draws[0])
            d.shading = model
            row = [d]
            if extra is not None:   # a second draw: one tiny triangle hidden inside Suzanne
                e = copy.copy(draws[0])
                e.mesh, e.shading = speck, extra
                row.append(e)
            out.append(row)
        return ctx.prepare_batch(frame, out)

    rows = [("blinn_phong", batch(3))] + [(names[m], batch(m)) for m in range(4, 9)] + \
           [("blinn_phong + speck", batch(3, 3)), ("blinn_phong (ext kernels)", batch(3, 4)), ("blinn_phong again", batch(3))]
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
    lines = [f"legacy shading models on C2: one batch of {FRAMES} poses at {frame.width}x{frame.height} per step "
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
