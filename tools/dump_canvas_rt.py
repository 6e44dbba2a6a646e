"""SHA-256 of every plane the Canvas render-target raster writes, for a bit-for-bit comparison of two builds of the library
(GPU box): run once per library, each in a process of its own, and diff the two outputs.

  tools/build_variant.sh base                                                       # the parent commit's library
  SHS_GPU_LIB=$PWD/leisure-software-renderer_amd/shs_gpu/libshs_base.so python tools/dump_canvas_rt.py > base.txt
  python tools/dump_canvas_rt.py > here.txt && diff base.txt here.txt

One small frame through every camera-pass shader: a 100x37 target with tile jobs of 16 -- ragged 32x8 raster tiles on both
edges, several reference jobs per tile -- over a 64x64 shadow map; a textured quad that passes under the camera (so the
near plane clips it), an untextured monkey that turns between the previous and the current frame, and a quad between the
two that casts on the first; SHS_RT_PREQUANT on.  The shadow pass, then shading 0 with and without the PCF, 1, 2 without and
with an IBL, 3, 4 under no sky / the analytic sky / a cubemap sky, and 5 without and with a kept reflection: per pass the
hash of the colour, depth, velocity, id and prequant planes.  Then a few hundred seeded points through the four *_samples
entries.  (The library's name is not printed: the outputs must diff empty.)"""
import dataclasses
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "leisure-software-renderer_amd"), ROOT, os.path.join(ROOT, "tools")]
import exp_canvas_rt as hard  # noqa: E402

W, H, TILE, SM = 100, 37, 16, 64
N_SAMPLES = 300


def sha(a):
    import numpy as np
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def quad(x0, x1, z0, z1, y):
    import numpy as np
    from shs_gpu import scene
    a, b, c, d = (x0, y, z0), (x1, y, z0), (x1, y, z1), (x0, y, z1)
    pos = np.array([np.concatenate([a, b, c]), np.concatenate([a, c, d])], np.float32)
    uv = np.array([[0, 0, 1, 0, 1, 1], [0, 0, 1, 1, 0, 1]], np.float32)
    return scene.Mesh(pos, np.tile(np.array([0, 1, 0] * 3, np.float32), (2, 1)), uv)


def scene_of():
    import numpy as np
    import shs_gpu
    from shs_gpu import scene
    frame, _ = hard.demo(0.0, 0.0)   # the hard demo's camera and light
    frame = dataclasses.replace(frame, width=W, height=H, ref_tile=(TILE, TILE), prequant=True)
    proj = scene.camera(frame.camera_pos, 0.0, 0.0)[1]
    vp = scene.mat_mul(proj, frame.view)
    eye = np.eye(4, dtype=np.float32).reshape(16)
    tex = hard.Texture(np.random.default_rng(2).integers(0, 256, (16, 16, 4), dtype=np.uint8))
    m_now = scene.model_trs((-4.0, 8.0, 0.0), 0.7, (6.0, 6.0, 6.0))
    m_prev = scene.model_trs((-4.0, 8.0, 0.0), 0.4, (6.0, 6.0, 6.0))
    draws = [shs_gpu.RtDraw(quad(-40.0, 40.0, -60.0, 80.0, 0.0), eye, vp, vp, (120, 122, 128, 255), tex),
             shs_gpu.RtDraw(scene.monkey(), m_now, scene.mat_mul(vp, m_now), scene.mat_mul(vp, m_prev), (180, 150, 95, 255)),
             shs_gpu.RtDraw(quad(-20.0, 6.0, -10.0, 20.0, 4.0), eye, vp, vp, (200, 60, 40, 255))]
    return frame, draws, proj


def main():
    import numpy as np

    import shs_gpu
    from shs_gpu import lib_path, scene
    ctx = shs_gpu.Context(0)
    frame, draws, proj = scene_of()
    rng = np.random.default_rng(3)

    def planes(name):
        color, depth, vel = ctx.rt_resolve()
        ids = ctx.rt_resolve_ids()
        print(f"{name}: colour {sha(color)}\n{name}: depth {sha(depth)}\n{name}: velocity {sha(vel)}\n"
              f"{name}: ids {sha(ids)} ({int((ids >= 0).sum())} shaded pixels of {W * H})\n{name}: prequant {sha(ctx.rt_resolve_prequant())}")

    ctx.rt_render_shadow(SM, frame.light_vp, draws, ref_tile=(TILE, TILE))
    shadow = ctx.rt_resolve_shadow()
    print(f"shadow pass: map {sha(shadow)}")
    for pcf in (True, False):
        ctx.rt_render(dataclasses.replace(frame, pcf=pcf), draws)
        planes(f"shading 0, pcf {int(pcf)}")
    ctx.rt_render(dataclasses.replace(frame, shading=1), draws)
    planes("shading 1")

    def n3(model):   # transpose(inverse(mat3(model))), column-major
        return np.linalg.inv(np.asarray(model, np.float64).reshape(4, 4).T[:3, :3]).astype(np.float32).reshape(9)
    mats = [shs_gpu.RtPbrDraw(None, 0.0, 0.70, 1.0, 1.30, 0.60, 0.20), shs_gpu.RtPbrDraw(n3(draws[1].model), 0.95, 0.20, 1.0, 1.00, 1.80, 1.00),
            shs_gpu.RtPbrDraw(None, 0.0, 0.22, 0.8, 1.50, 1.00, 1.20)]
    irr = rng.uniform(0.0, 4.0, (6, 4, 4, 3)).astype(np.float32)
    spec = [rng.uniform(0.0, 4.0, (6, 16 >> m, 16 >> m, 3)).astype(np.float32) for m in range(4)]
    ctx.rt_render_pbr(dataclasses.replace(frame, shading=2), draws, mats)
    planes("shading 2, no ibl")
    ctx.rt_set_ibl(irr, spec)
    ctx.rt_render_pbr(dataclasses.replace(frame, shading=2), draws, mats)
    planes("shading 2, ibl")
    ctx.rt_render_pbr_soft(dataclasses.replace(frame, shading=3), draws, mats)
    planes("shading 3, ibl")

    faces = tuple(ctx.upload_texture(hard.Texture(rng.integers(0, 256, (8, 8, 4), dtype=np.uint8))) for _ in range(6))
    skies = {"none": None, "analytic": shs_gpu.RtSky(model=1, encode=1), "cubemap": shs_gpu.RtSky(model=2, encode=1, face_tex=faces)}
    knobs = [shs_gpu.RtSkyboxIblDraw(0.30, 0.22, 0.04, 0.10), shs_gpu.RtSkyboxIblDraw(0.28, 0.38, 0.04, 0.60),
             shs_gpu.RtSkyboxIblDraw(0.30, 0.32, 0.04, 0.35)]
    dirs = rng.normal(size=(N_SAMPLES, 3)).astype(np.float32)
    for name, sky in skies.items():
        ctx.rt_set_sky(sky)
        ctx.rt_render_skybox_ibl(dataclasses.replace(frame, shading=4), draws, knobs)
        planes(f"shading 4, sky {name}")
        if sky is not None:
            print(f"sky samples, {name}: {sha(ctx.rt_sky_samples(dirs))}")
    ctx.rt_set_sky(None)

    # hello_water.cpp's frame: the quad is the water, mirrored at its height for the reflection pass
    flags = [shs_gpu.RtWaterDraw(i == 0) for i in range(len(draws))]
    water = dataclasses.replace(frame, shading=5)
    ctx.rt_render_water(water, draws, flags, shs_gpu.RtWater(None, 1.3, False))
    planes("shading 5, no reflection")
    cam = frame.camera_pos
    mpos = (cam[0], -cam[1], cam[2])
    rview = lib_path.look_at_lh(mpos, (mpos[0], mpos[1], mpos[2] + 1.0), (0.0, -1.0, 0.0))
    rvp = scene.mat_mul(proj, rview)
    objs = [dataclasses.replace(d, mvp=scene.mat_mul(rvp, d.model), prev_mvp=scene.mat_mul(rvp, d.model)) for d in draws[1:]]
    ctx.rt_render_water(dataclasses.replace(water, view=rview, camera_pos=mpos), objs, [shs_gpu.RtWaterDraw(False)] * len(objs),
                        shs_gpu.RtWater(None, 1.3, False))
    planes("shading 5, the reflection pass")
    ctx.rt_keep_reflection()
    ctx.rt_render_water(water, draws, flags, shs_gpu.RtWater(rvp, 1.3, True))
    planes("shading 5, kept reflection")

    uv = rng.uniform(-0.05, 1.05, (N_SAMPLES, 2)).astype(np.float32)
    z = rng.uniform(0.0, 1.0, N_SAMPLES).astype(np.float32)
    bias = rng.uniform(0.0, 0.01, N_SAMPLES).astype(np.float32)
    pxpy = rng.integers(0, 100, (N_SAMPLES, 2)).astype(np.int32)
    print(f"pcss samples: {sha(ctx.rt_pcss_samples(shadow, uv, z, bias, pxpy))}")
    a, b = ctx.rt_ibl_samples(dirs, rng.uniform(-0.5, 4.5, N_SAMPLES).astype(np.float32))
    print(f"ibl samples: irradiance {sha(a)}, specular {sha(b)}")
    nrm, foam = ctx.rt_water_samples(rng.uniform(-60.0, 60.0, (N_SAMPLES, 3)).astype(np.float32), 1.3)
    print(f"water samples: normal {sha(nrm)}, foam {sha(foam)}")
    print(f"last pass: {ctx.rt_stats()}")


if __name__ == "__main__":
    main()
