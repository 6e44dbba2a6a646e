"""Sky model backgrounds at 4K (GPU box): the C5 camera pass with the gradient, a ProceduralSky and a
CubemapSky (six 512x512 faces) behind the meshes, product library, against the parent commit's gradient
frame.

  tools/build_variant.sh base            # shs_gpu/libshs_base.so from HEAD~1 (no GPU needed)
  python tools/exp_sky.py profiles/sky_4k.txt

The parent process never opens the GPU: it starts one child per (library, repetition), base and branch
interleaved (as tools/ab.sh does), each under its own time limit, and stops at the first failure.  A child
times the whole camera pass (setup, raster, resolve) with one event pair per frame on the context stream:
median of RUNS frames after WARM warm-up frames.  The branch's first child also checks the two sky frames
against tests/sky_ref (uncovered pixels bit-equal to the restatement's fill, everything else bit-equal to the
gradient frame).  The base library has no sky entry points: its child times the gradient frame only.

The design not chosen -- a sky pass of its own that writes the HDR target and lets the resolve read it back --
moves 2 x W*H*16 B; at the ~6.0 TB/s plain-store rate VERDICT.md records that is the figure printed beside the
measured excess."""
import ctypes
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "leisure-software-renderer_amd")
W, H = (int(os.environ.get("SKY_W", 3840)), int(os.environ.get("SKY_H", 2160)))
RUNS, WARM = int(os.environ.get("SKY_RUNS", 200)), int(os.environ.get("SKY_WARM", 60))
REPS = int(os.environ.get("SKY_REPS", 2))
FACE = 512
SUN_AT = (3.0, 8.5, 4.0)     # the sun lies behind this point: in the sky right of Suzanne, above the floor's far edge
STORE_TBS = 6.0              # plain-store ceiling


def child(check):
    sys.path[:0] = [PKG, ROOT, os.path.join(ROOT, "tests")]
    import numpy as np
    import torch
    from shs_gpu import _abi
    probe = ctypes.CDLL(os.environ["SHS_GPU_LIB"]) if os.environ.get("SHS_GPU_LIB") else None
    has_sky = probe is None or hasattr(probe, "shs_lib_set_sky")
    if probe is not None:   # the parent commit's library: bind what it has
        _abi.SIGNATURES[:] = [s for s in _abi.SIGNATURES if hasattr(probe, s[0])]
    import shs_gpu
    from shs_gpu import scene_lib
    from shs_gpu.lib_path import LibSky, Texture2D

    frame, draws, _casters, _sun, _S = scene_lib.c5_scene(W, H)
    vp, eye = np.asarray(draws[0].viewproj, np.float32), tuple(draws[0].camera_pos)
    d = np.asarray(SUN_AT, np.float64) - np.asarray(eye, np.float64)
    rng = np.random.default_rng(512)
    skies = {"procedural": LibSky(model=1, cam_viewproj=vp, cam_pos=eye, sun_dir_ws=tuple(float(v) for v in -d / np.linalg.norm(d))),
             "cubemap": LibSky(model=2, cam_viewproj=vp, cam_pos=eye, intensity=1.5,
                               faces=[Texture2D(rng.integers(0, 256, size=(FACE, FACE, 4), dtype=np.uint8)) for _ in range(6)])}
    ctx = shs_gpu.Context(0)
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    ctx.set_stream(stream.cuda_stream)
    prepared = ctx.prepare_lib(frame, draws)
    out = {"lib": os.path.basename(os.environ.get("SHS_GPU_LIB", "libshs_gpu.so"))}
    # one frame with its statistics read, in every child: the later passes then take the shallow raster (C5's
    # fullest bin tile fits one round), as a host that reads its statistics gets it
    ctx.render_pbr_forward_prepared(prepared)
    out["covered_px"] = ctx.lib_stats()["covered_pixels"]

    def timed():
        for _ in range(WARM):
            ctx.render_pbr_forward_prepared(prepared)
        torch.cuda.synchronize()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(RUNS)]
        for a, b in ev:
            a.record()
            ctx.render_pbr_forward_prepared(prepared)
            b.record()
        torch.cuda.synchronize()
        us = [a.elapsed_time(b) * 1e3 for a, b in ev]
        return [statistics.median(us), min(us), max(us)]

    if check and has_sky:
        import test_sky as ref
        ctx.render_pbr_forward_prepared(prepared)
        plain = ctx.resolve_lib()
        covered = plain[1] < 1.0
        for name, sky in skies.items():
            ctx.set_sky(sky)
            ctx.render_pbr_forward_prepared(prepared)
            want = ref.ref_fill(sky, W, H)
            ref._assert_sky_frame(ctx.resolve_lib(), plain, want, name)
            if name == "procedural":
                out["disc_px"] = int(((want[..., 0] == 15) & ~covered).sum())
                assert out["disc_px"] > 1000
        ctx.set_sky(None)
        out["checked"] = f"sky frames equal tests/sky_ref bit for bit ({int((~covered).sum())} uncovered pixels)"
    out["gradient"] = timed()
    if has_sky:
        for name, sky in skies.items():
            ctx.set_sky(sky)
            out[name] = timed()
        ctx.set_sky(None)
        out["gradient_again"] = timed()
    ctx.close()
    print("RESULT " + json.dumps(out), flush=True)


def main():
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    libs = [("base", os.path.join(PKG, "shs_gpu", "libshs_base.so")), ("branch", os.path.join(PKG, "shs_gpu", "libshs_gpu.so"))]
    for _, so in libs:
        if not os.path.exists(so):
            sys.exit(f"{so} missing (tools/build_variant.sh base; the product build)")
    say(f"sky model backgrounds, C5 camera pass {W}x{H} (no shadow pass), us per frame: median of {RUNS} (min-max) after {WARM} "
        f"warm-up frames; one process per row, base = the parent commit's library")
    res = {"base": [], "branch": []}
    for rep in range(REPS):
        for name, so in libs:
            env = dict(os.environ, SHS_GPU_LIB=so)
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"] + (["--check"] if rep == 0 else []),
                               env=env, capture_output=True, text=True, timeout=400)
            got = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
            if p.returncode != 0 or not got:
                sys.exit(f"{name} rep {rep}: exit {p.returncode}\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}")
            r = json.loads(got[0][7:])
            res[name].append(r)
            if "checked" in r:
                say(f"{r['checked']}; {r['disc_px']} sun disc pixels")
            for k in ("gradient", "procedural", "cubemap", "gradient_again"):
                if k in r:
                    say(f"  {name:6s} run {rep + 1}  {k:15s} {r[k][0]:7.1f} ({r[k][1]:.1f}-{r[k][2]:.1f})")
    base = [r["gradient"][0] for r in res["base"]]
    spread = max(base) - min(base)
    b = statistics.mean(base)
    say(f"parent gradient frame: {b:.1f} us, spread of its {len(base)} runs {spread:.1f} us")
    g = [r[k][0] for r in res["branch"] for k in ("gradient", "gradient_again")]
    say(f"branch gradient frame: {statistics.mean(g):.1f} us ({min(g):.1f}-{max(g):.1f} over {len(g)} windows): "
        f"{statistics.mean(g) - b:+.1f} us against the parent")
    alt_us = 2 * W * H * 16 / (STORE_TBS * 1e12) * 1e6
    for k in ("procedural", "cubemap"):
        v = [r[k][0] for r in res["branch"]]
        own = [r[k][0] - (r["gradient"][0] + r["gradient_again"][0]) / 2 for r in res["branch"]]
        say(f"{k} sky frame: {statistics.mean(v):.1f} us ({min(v):.1f}-{max(v):.1f}): {statistics.mean(v) - b:+.1f} us over the parent's "
            f"gradient frame ({', '.join(f'{o:+.1f}' for o in own)} over the same process's); a separate sky pass would write and "
            f"re-read 2 x {W * H * 16 / 1e6:.1f} MB = {alt_us:.0f} us at {STORE_TBS} TB/s")
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    if "--child" in sys.argv:
        child("--check" in sys.argv)
    else:
        main()
