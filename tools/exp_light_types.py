"""Cost of the typed Forward+ program on the full-size C4 scene (GPU box).

usage: python tools/exp_light_types.py [frames] [rounds]
Per-frame ms (light cull + camera pass, wall clock over `frames` frames after a warm-up) of
  (a) program 5 with the C4 point set (shs_lights_upload),
  (b) program 6 with the same point set uploaded typed (the cost of the typed kernel on point lights),
  (c) program 6 with scene_lib.c4_lights_typed (the cost of the spot / rect / tube models),
interleaved a, b, c per round on three contexts of device 0; the rounds show each configuration's spread."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "leisure-software-renderer_amd"), ROOT]
import numpy as np  # noqa: E402
import shs_gpu  # noqa: E402
from shs_gpu import lib_path, scene_lib  # noqa: E402


def main():
    frames = int(sys.argv[1]) if len(sys.argv) > 1 else 30
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    frame, draws5, lights, cull = scene_lib.c4_scene()
    draws6 = [type(d)(**{**d.__dict__, "program": lib_path.PROGRAM_FORWARD_PLUS_TYPED}) for d in draws5]
    points = scene_lib.c4_lights_typed(len(lights))
    points["type"] = lib_path.LIGHT_POINT
    configs = [("a: program 5, point set", draws5, lambda c: c.upload_lights(lights)),
               ("b: program 6, point set typed", draws6, lambda c: c.upload_lights_typed(points)),
               ("c: program 6, mixed types", draws6, lambda c: c.upload_lights_typed(scene_lib.c4_lights_typed(len(lights))))]
    runs = []
    for label, draws, upload in configs:
        ctx = shs_gpu.Context(0)
        upload(ctx)
        ctx.light_cull(cull)
        prepared = ctx.prepare_lib(frame, draws)
        for _ in range(3):
            ctx.light_cull(cull)
            ctx.render_pbr_forward_prepared(prepared)
        ctx.synchronize_lib()
        runs.append((label, ctx, prepared, []))
    for _ in range(rounds):
        for label, ctx, prepared, ms in runs:
            t0 = time.perf_counter()
            for _ in range(frames):
                ctx.light_cull(cull)
                ctx.render_pbr_forward_prepared(prepared)
            ctx.synchronize_lib()
            ms.append((time.perf_counter() - t0) / frames * 1e3)
    for label, ctx, _, ms in runs:
        counts = ctx.resolve_light_lists()[0]
        ctx.close()
        print(f"{label:32s} median {np.median(ms):7.3f} ms  min {min(ms):7.3f}  max {max(ms):7.3f}  rounds "
              + " ".join(f"{m:.3f}" for m in ms) + f"  | lists mean {counts.mean():.1f} max {counts.max()}", flush=True)


if __name__ == "__main__":
    main()
