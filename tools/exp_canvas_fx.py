"""The Canvas-API post passes (shs_canvas_velocity_blur, _fog, _outline, _fxaa, _spec_bright, _additive, _lens_flare) and
the two frame entries (shs_canvas_multi_pass_frame, shs_canvas_glow_frame) timed on the GPU box, at the demos' 380x280
canvas and at 1200x900.

  python tools/exp_canvas_fx.py profiles/canvas_fx.txt   # appends its lines to the file
  python tools/exp_canvas_fx.py - trace 0                # size 0 (or 1) alone: the frames, then every pass LAUNCHES times,
                                                         # without events, for a `rocprofv3 --kernel-trace -- python ...`
                                                         # run (tools/kstats.py DIR "" --last 200: the passes' own launches)

One context on one stream; every call goes straight to the C entry with a desc and pointers built once, so the host
adds a ctypes call per launch and nothing else.  After a clock ramp (RAMP frame chains) and WARM warm-up launches, each
pass is timed RUNS times: one device event pair around LAUNCHES back-to-back launches, divided by LAUNCHES.  That is
what a pass costs in a stream of dependent launches -- kernel, launch gap and, where the host is the slower side, the
enqueue -- and not the kernel alone; the kernels' own durations come from the kernel trace (above).  The frames are
timed the same way on device buffers, and through host buffers with the host clock around the synchronous call."""
import ctypes
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "leisure-software-renderer_amd"), ROOT]

SIZES = ((380, 280), (1200, 900))
RAMP, WARM, LAUNCHES, RUNS = 60, 20, 200, 8
# bytes a pixel must move at least (read + written; the neighbour taps hit the caches): colour 4, depth 4, velocity 8
BYTES = {"velocity_blur": 16, "fog": 12, "outline": 12, "fxaa": 8, "spec_bright": 8, "additive": 12, "lens_flare": 8,
         "gaussian (one axis)": 8}
HBM = 6.3e12      # achievable bytes / s (the float4-copy figure)


def inputs(w, h):
    import numpy as np
    rng = np.random.default_rng(w * 1000 + h)
    yy, xx = np.mgrid[0:h, 0:w]
    src = rng.integers(0, 256, (h, w, 4)).astype(np.uint8)
    src[:, : w // 2] = (90, 140, 200, 255)
    depth = (5.0 + 95.0 * (xx + yy) / (w + h - 2)).astype(np.float32)
    depth[rng.random((h, w)) < 0.1] = np.finfo(np.float32).max
    vel = rng.normal(0.0, 6.0, (h, w, 2)).astype(np.float32)
    spec = (rng.random((h, w)) ** 3 * 1.2).astype(np.float32)
    return src, depth, vel, spec


def main():
    import numpy as np
    import torch

    import shs_gpu
    out = sys.argv[1] if len(sys.argv) > 1 else "-"
    trace = len(sys.argv) > 2 and sys.argv[2] == "trace"
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    ctx = shs_gpu.Context(0)
    ctx.set_stream(stream.cuda_stream)
    lines = [f"exp_canvas_fx: {LAUNCHES} launches x {RUNS} runs after {RAMP} frame chains + {WARM} launches; us per launch "
             f"(median of the runs; min .. max of the runs)"]

    def timed(fn):
        per = []
        for _ in range(RUNS):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(LAUNCHES):
                fn()
            e1.record(stream)
            ctx.synchronize()
            per.append(e0.elapsed_time(e1) * 1e3 / LAUNCHES)
        return statistics.median(per), min(per), max(per)

    def host_timed(fn, n=40):
        meds = []
        for _ in range(RUNS):
            t = []
            for _ in range(n):
                t0 = time.perf_counter()
                fn()
                t.append((time.perf_counter() - t0) * 1e6)
            meds.append(statistics.median(t))
        return statistics.median(meds), min(meds), max(meds)

    sizes = SIZES if len(sys.argv) <= 3 else (SIZES[int(sys.argv[3])],)
    for w, h in sizes:
        src, depth, vel, spec = inputs(w, h)
        t = lambda a: torch.from_numpy(a).cuda()
        d_src, d_depth, d_vel, d_spec = t(src), t(depth), t(vel), t(spec)
        d_out, d_out2 = torch.empty_like(d_src), torch.empty_like(d_src)
        bloom = ctx.canvas_spec_bright(d_spec)
        bloom = ctx.canvas_gaussian_blur(ctx.canvas_gaussian_blur(bloom, True), False)
        L, DEV, ref = ctx._lib, ctx.CANVAS_DEVICE, ctypes.byref
        P = lambda a: ctypes.c_void_p(a.data_ptr() if hasattr(a, "data_ptr") else a.ctypes.data)
        descs = {k: ctx.fx_desc(k, w, h) for k in ("velocity_blur", "fog", "outline", "fxaa", "spec_bright", "lens_flare")}
        descs["multi"], descs["glow"] = ctx.multi_pass_frame_desc(w, h), ctx.glow_frame_desc(w, h)

        def call(fn, *args):
            def run():
                ctx._check(fn(ctx._h, *args))
            return run
        passes = {
            "velocity_blur": call(L.shs_canvas_velocity_blur, ref(descs["velocity_blur"]), P(d_src), P(d_vel), P(d_out), DEV),
            "fog": call(L.shs_canvas_fog, ref(descs["fog"]), P(d_src), P(d_depth), P(d_out), None, DEV),
            "outline": call(L.shs_canvas_outline, ref(descs["outline"]), P(d_src), P(d_depth), P(d_out), DEV),
            "fxaa": call(L.shs_canvas_fxaa, ref(descs["fxaa"]), P(d_src), P(d_out), DEV),
            "spec_bright": call(L.shs_canvas_spec_bright, ref(descs["spec_bright"]), P(d_spec), P(d_out), DEV),
            "additive": call(L.shs_canvas_additive, w, h, P(d_src), P(bloom), 1.0, P(d_out), DEV),
            "lens_flare": call(L.shs_canvas_lens_flare, ref(descs["lens_flare"]), P(bloom), P(d_out), None, DEV),
            "gaussian (one axis)": call(L.shs_canvas_gaussian_blur, w, h, P(d_src), P(d_out), 1, DEV),
        }
        host_out = np.empty_like(src)
        frames = {
            "multi_pass_frame (6 + 8 Gaussian launches)": call(L.shs_canvas_multi_pass_frame, ref(descs["multi"]), P(d_src), P(d_depth),
                                                               P(d_vel), P(d_out2), DEV),
            "glow_frame (7 + 26 Gaussian launches)": call(L.shs_canvas_glow_frame, ref(descs["glow"]), P(d_src), P(d_depth), P(d_vel),
                                                          P(d_spec), P(d_out2), DEV),
        }
        host_frames = {
            "multi_pass_frame, host buffers": call(L.shs_canvas_multi_pass_frame, ref(descs["multi"]), P(src), P(depth), P(vel),
                                                   P(host_out), 0),
            "glow_frame, host buffers": call(L.shs_canvas_glow_frame, ref(descs["glow"]), P(src), P(depth), P(vel), P(spec),
                                             P(host_out), 0),
        }
        for _ in range(RAMP):
            for fn in frames.values():
                fn()
        for fn in list(passes.values()) + list(frames.values()):
            for _ in range(WARM):
                fn()
        ctx.synchronize()
        if trace:
            for fn in list(frames.values()) + list(passes.values()):
                for _ in range(LAUNCHES):
                    fn()
            ctx.synchronize()
            continue
        lines.append(f"  {w}x{h} ({w * h} pixels)")
        for name, fn in passes.items():
            med, lo, hi = timed(fn)
            floor = w * h * BYTES[name] / HBM * 1e6
            lines.append(f"    {name:22s} {med:7.2f}  ({lo:.2f} .. {hi:.2f})   {BYTES[name]:2d} B/px: {floor:.2f} us at {HBM / 1e12:.1f} TB/s, "
                         f"{w * h * BYTES[name] / (med * 1e-6) / 1e9:.0f} GB/s achieved")
        for name, fn in frames.items():
            med, lo, hi = timed(fn)
            lines.append(f"    {name:44s} {med:8.1f}  ({lo:.1f} .. {hi:.1f})   device buffers, per frame of a back-to-back stream")
        for name, fn in host_frames.items():
            med, lo, hi = host_timed(fn)
            lines.append(f"    {name:44s} {med:8.1f}  ({lo:.1f} .. {hi:.1f})   host clock, copies in and out included")
    text = "\n".join(lines)
    print(text)
    if out != "-" and not trace:
        with open(os.path.join(ROOT, out) if not os.path.isabs(out) else out, "a") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
