"""PassLightShafts at 4K (GPU box): C5 frame, sun aimed at (0, 1.5, 0), default parameters.

Times k_shaft_mask and k_light_shafts separately with events on the context stream (median of RUNS
launches after a warm-up that also ramps the clock), the product call (both kernels), k_motion_blur on
the same frame as the yardstick (10 taps, two gathers per tap) and the C restatement's single-thread CPU
time.  Checks the bytes against the restatement first.

Needs the timing-experiments build (make -C leisure-software-renderer_amd exp): SHS_LS_PART (1 the mask
kernel alone, 2 the march alone) is read by it only, and only it lets the pass run again on the same
tonemap (the timed launches shaft an already shafted LDR: same work, other bytes).  The workgroup pixel
shapes in profiles/light_shafts_4k.txt were timed with a build that had k_light_shafts as a template over
them.  Usage: python tools/exp_light_shafts.py [out_file]"""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "leisure-software-renderer_amd")
os.environ.setdefault("SHS_GPU_LIB", os.path.join(PKG, "shs_gpu", "libshs_gpu_exp.so"))
sys.path[:0] = [PKG, ROOT, os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402
import torch  # noqa: E402
import shs_gpu  # noqa: E402
from shs_gpu import scene_lib  # noqa: E402
import test_light_shafts as ref  # noqa: E402  (the restatement's ctypes binding)

W, H = (int(os.environ.get("LS_W", 3840)), int(os.environ.get("LS_H", 2160)))
RUNS, WARM = int(os.environ.get("LS_RUNS", 60)), 30
STEPS = 48
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def timed(fn, runs=RUNS, warm=WARM):
    """Median / min / max ms of `fn`'s stream work: one event pair per launch."""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(runs)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    ms = [a.elapsed_time(b) for a, b in ev]
    return statistics.median(ms), min(ms), max(ms)


frame, draws, _casters, _sun, _S = scene_lib.c5_scene(W, H)
vp, eye = np.asarray(draws[0].viewproj, np.float32), np.asarray(draws[0].camera_pos, np.float32)
sun = ref._aim(eye, (0.0, 1.5, 0.0))
px = W * H
ctx = shs_gpu.Context(0)
stream = torch.cuda.Stream()          # a real stream: torch's default one is the null stream
torch.cuda.set_stream(stream)
ctx.set_stream(stream.cuda_stream)
say(f"PassLightShafts {W}x{H} C5, sun_uv {ref.ref_sun_uv(vp, eye, sun)[0]}, steps {STEPS}, median of {RUNS} "
    f"(min-max), {WARM} warm-up launches; library {os.path.basename(os.environ['SHS_GPU_LIB'])}")

# the bytes against the restatement (and its single-thread CPU time)
ctx.render_pbr_forward(frame, draws)
ctx.tonemap(1.0, 2.2, ldr=True, present=True)
base, _ = ctx.resolve_ldr()
_, depth, _ = ctx.resolve_lib()
t0 = time.perf_counter()
want, boost, ran = ref.ref_shafts(base, depth, vp, eye, sun)
cpu_s = time.perf_counter() - t0
assert ran
ctx.light_shafts(vp, eye, sun)
got, pre = ctx.resolve_ldr()
assert np.array_equal(got, want) and np.array_equal(pre, want[::-1])
say(f"bytes equal the restatement's; boost: {len(np.unique(boost))} values, "
    f"{((boost == 0) | (boost == 120)).mean():.2f} of the pixels at 0 or 120")
say(f"restatement, one CPU thread: {cpu_s * 1e3:.0f} ms ({px * STEPS / cpu_s / 1e6:.0f} Mtaps/s)")

os.environ["SHS_LS_PART"] = "1"
ms, lo, hi = timed(lambda: ctx.light_shafts(vp, eye, sun))
by = px * 12                           # 4 B LDR + 4 B depth read, 4 B mask written
say(f"k_shaft_mask: {ms * 1e3:.1f} us ({lo * 1e3:.1f}-{hi * 1e3:.1f}), {by / ms / 1e6:.0f} GB/s of its 12 B/px = "
    f"{by / ms / 1e6 / 6300:.2f} of the 6.3 TB/s achievable HBM rate ({by / ms / 1e6 / 8000:.2f} of the 8 TB/s peak)")
os.environ["SHS_LS_PART"] = "2"
ms, lo, hi = timed(lambda: ctx.light_shafts(vp, eye, sun))
say(f"k_light_shafts: {ms * 1e3:.1f} us ({lo * 1e3:.1f}-{hi * 1e3:.1f}), {px * STEPS / ms / 1e6:.1f} Gtaps/s, "
    f"{ms * 1e6 / (px * STEPS) * 1e3:.2f} ps/tap")
del os.environ["SHS_LS_PART"]
ms, lo, hi = timed(lambda: ctx.light_shafts(vp, eye, sun))
say(f"shs_light_shafts (both kernels): {ms * 1e3:.1f} us ({lo * 1e3:.1f}-{hi * 1e3:.1f}); "
    f"CPU restatement / GPU = {cpu_s * 1e3 / ms:.0f}x")

# the yardstick: PassMotionBlur's default 10 taps, each a depth and a colour gather (min_velocity 0: every pixel taps)
ctx.tonemap(1.0, 2.2, ldr=True, present=False)
ms, lo, hi = timed(lambda: ctx.motion_blur(present=False, min_velocity_px=0.0))
say(f"k_motion_blur (10 taps x 2 gathers): {ms * 1e3:.1f} us ({lo * 1e3:.1f}-{hi * 1e3:.1f}), {px * 10 / ms / 1e6:.1f} Gtaps/s, "
    f"{ms * 1e6 / (px * 10) * 1e3:.2f} ps/tap")
ctx.close()
if len(sys.argv) > 1:
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
    with open(sys.argv[1], "w") as f:
        f.write("\n".join(lines) + "\n")
