"""tests/canvas_rt_plain_ref (ref_canvas_rt_plain.c), the C restatement of the camera passes of
hello_per_object_motion_blur.cpp (shading 8), hello_depth_of_field.cpp (9) and hello_ping_pong.cpp (10) and of the first
demo's post_process_motion_blur -- the reference of tests/test_canvas_rt_plain.py -- pinned on the CPU:

  * against a float32 numpy witness of the whole pass (np_render_plain) and of the blur (np_object_blur), written from
    the same cited lines and vectorised per triangle / per sample index, on every scene and blur input of the GPU tests:
    ids, depth and velocity bit for bit, the colour under helpers.assert_color_parity, the blur's bytes equal;
  * by hand-computed known answers: a screen-filling triangle's depth (view z and NDC z), its row in the depth plane and
    its velocity at a named pixel; one blur pixel's samples, with and without a rejected one;
  * test_rule_swaps_change_pixels: the witness with one rule swapped for its neighbour's (shading 6's ambient, a depth
    plane in canvas rows, view z for shading 10, frag_velocity's clamped screen difference, a [0, 1] kernel, no depth
    rejection, the other depth_rows) changes pixels on the scene named beside it, so a kernel that kept that rule cannot
    pass.

It also holds what fails without the feature and needs no GPU: the library's new entry points, the header's
declarations and the new desc's size.

The depth plane of these three shadings is in SCREEN rows (the demos hand ZBuffer::test_and_set_depth the screen py);
every other plane is in canvas rows."""
import ctypes
import dataclasses
import functools
import os
import subprocess

import numpy as np
import pytest

import helpers
import test_canvas_rt_motion_ref as M
import test_canvas_rt_pbr_ref as P
import test_canvas_rt_ref as R
import test_sky as SK
from test_canvas_rt_ref import F, FLT_MAX

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REF_DIR = os.path.join(HERE, "canvas_rt_plain_ref")
REF_LIB = os.path.join(REF_DIR, "_build", "libshs_canvas_rt_plain_ref.so")
_P = ctypes.c_void_p
PX_ZTIE = 4
BAR = helpers.TOL * 255.0
EYE = M.EYE
W, H = 160, 120            # jobs of 80 x 80
WO, HO = 75, 53            # odd in both axes, aligned to neither the 32 x 8 raster tile nor jobs of 16 x 16
INT_MIN = -2 ** 31


class PlainPlanes(ctypes.Structure):
    _fields_ = [("color", _P), ("depth", _P), ("velocity", _P), ("prequant", _P), ("tri_id", _P), ("flags", _P),
                ("counters", ctypes.c_int64 * 4)]


@functools.lru_cache(maxsize=None)
def ref_lib():
    subprocess.run(["make", "-s", "-C", REF_DIR], check=True)
    L = ctypes.CDLL(REF_LIB)
    L.rcp_render.restype = ctypes.c_int
    L.rcp_render.argtypes = [ctypes.POINTER(R.RefFrame), ctypes.c_int32, ctypes.POINTER(R.RefDraw), ctypes.c_int, ctypes.POINTER(PlainPlanes)]
    L.rcp_object_blur.restype = ctypes.c_int
    L.rcp_object_blur.argtypes = [ctypes.c_int, ctypes.c_int, _P, _P, _P, _P, ctypes.c_float, ctypes.c_float, ctypes.c_float, ctypes.c_int,
                                  ctypes.c_float, ctypes.c_int]
    return L


def ref_render_plain(frame, draws):
    """The pass of a shs_gpu.RtFrame with shading 8, 9 or 10 -> the planes (depth in screen rows, the rest in canvas rows)
    and counters."""
    Wd, Hd = frame.width, frame.height
    keep = []
    arr = R._ref_draws(draws, keep)
    f = R.RefFrame()
    f.W, f.H = Wd, Hd
    f.tile_w, f.tile_h = frame.ref_tile
    for k in range(4):
        f.clear[k] = frame.clear_color[k]
    f.view[:] = [float(v) for v in np.asarray(frame.view, F).reshape(16)]
    f.light_dir[:] = [float(v) for v in frame.light_dir_world]
    f.camera_pos[:] = [float(v) for v in frame.camera_pos]
    f.max_velocity_px = frame.max_velocity_px
    out = {"color": np.empty((Hd, Wd, 4), np.uint8), "depth": np.empty((Hd, Wd), F), "velocity": np.empty((Hd, Wd, 2), F),
           "prequant": np.empty((Hd, Wd, 4), F), "tri_id": np.empty((Hd, Wd), np.int32), "flags": np.empty((Hd, Wd), np.int32)}
    p = PlainPlanes()
    for k, v in out.items():
        setattr(p, k, v.ctypes.data)
    assert ref_lib().rcp_render(ctypes.byref(f), frame.shading, arr, len(draws), ctypes.byref(p)) == 0
    out["counters"] = dict(zip(("input_tris", "polys3", "polys4", "sub_tris"), (int(c) for c in p.counters)))
    return out


def blur_params(**over):
    import shs_gpu
    return dict(shs_gpu.Context.FX_DEFAULTS["object_blur"], **over)


def ref_object_blur(src, depth, velocity, **over):
    """post_process_motion_blur restated -> (dst, the number of pixels that gathered)."""
    p = blur_params(**over)
    src = np.ascontiguousarray(src, np.uint8)
    depth, velocity = np.ascontiguousarray(depth, F), np.ascontiguousarray(velocity, F)
    Hd, Wd = depth.shape
    dst = np.empty_like(src)
    n = ref_lib().rcp_object_blur(Wd, Hd, src.ctypes.data, depth.ctypes.data, velocity.ctypes.data, dst.ctypes.data, p["multiplier"],
                                  p["velocity_scale"], p["min_vel2"], p["max_samples"], p["depth_eps"], p["depth_rows"])
    return dst, n


# ---- scenes (shared with tests/test_canvas_rt_plain.py) ---------------------------------------------------------

def plain_frame(view, shading, w=W, h=H, tile=(80, 80), **kw):
    return M.motion_frame(view, shading, w=w, h=h, tile=tile, **kw)


@functools.lru_cache(maxsize=None)
def part_monkey(n=150):
    """The first n triangles of the test mesh (both windings towards any camera)."""
    from shs_gpu import scene
    m = scene.monkey()
    return R.SoupMesh(m.positions[:n], m.normals[:n])


def scene_demo(shading, w=W, h=H, tile=(80, 80)):
    """The demos in miniature, asymmetric top to bottom: a part of the monkey high on the left that moved and turned, one
    low on the right at rest (prev_mvp == mvp: its velocity is exactly zero), and a far wall behind the lower two thirds of
    the frame that slid sideways.  302 triangles, 604 records: the raster runs three rounds."""
    from shs_gpu import scene
    view, proj = R.camera(w, h)
    s = (2.6, 2.6, 2.6)
    draws = [R._rt_draw(part_monkey(), scene.model_trs((-2.6, 3.2, 2.0), 25.0, s), view, proj,
                        prev_model=scene.model_trs((-2.0, 3.0, 2.0), 10.0, s), color=(60, 100, 200, 255)),
             R._rt_draw(part_monkey(), scene.model_trs((2.8, 0.6, 0.5), -30.0, s), view, proj, color=(200, 90, 80, 255)),
             R._rt_draw(R.quad_xy(-9.0, 9.0, -3.0, 3.0, 9.0, flip=True), EYE, view, proj, prev_model=scene.model_trs((0.7, 0.0, 0.0), 0.0, (1.0, 1.0, 1.0)),
                        color=(80, 200, 120, 255))]
    return plain_frame(view, shading, w=w, h=h, tile=tile), draws


def scene_windings(shading=9):
    frame, draws = M.scene("windings")
    return dataclasses.replace(frame, shading=shading), draws


def scene_behind(shading=8):
    """test_canvas_rt_motion_ref.behind_mesh: triangle 0 has a corner at w = -0.5, so the interpolated w runs through zero
    inside it (Inf / NaN velocities where a pixel centre meets it, huge ones beside); triangle 1 a corner at w = 0."""
    frame, draws = M.scene("behind")
    return dataclasses.replace(frame, shading=shading), draws


def scene_prev_behind():
    frame, draws = M.scene("prev_behind")
    return dataclasses.replace(frame, shading=8), draws


def scene_coincident(shading=8):
    frame, draws = M.scene("coincident")
    return dataclasses.replace(frame, shading=shading), draws


def scene_w_zero_line():
    """One triangle on the odd frame under one job whose interpolated clip w is exactly zero at pixel centres: under NEAR_M
    (clip = (x, y, z, z + 1)) the corners (-1, 1, 0), (1, 1, 0), (7, 7, -8) have w = 1, 1, -7 and land on the screen at
    (0, 0), (74, 0) and, mirrored, (0, 52).  The barycentric of the third corner is (py + 0.5) / 52 = 1 / 8 exactly in screen
    row 6, where w = 7 / 8 - 7 / 8; at px = 18 and 55 the other two are 5 / 8, 1 / 4 and 1 / 8, 3 / 4, exact as well.  x / 0
    there is Inf, and with prev_mvp == mvp the difference is NaN; beside the line the velocities are finite and huge."""
    n = np.tile(np.array([0, 0, -1] * 3, F), (1, 1))
    mesh = R.SoupMesh(np.array([[-1, 1, 0, 1, 1, 0, 7, 7, -8]], F), n)
    return plain_frame(EYE, 8, w=WO, h=HO, tile=(WO, HO), cam_pos=(0.0, 0.0, -3.0)), [M.clip_draw(mesh)]


def scene_hair(tile):
    """test_canvas_rt_ref.hair_soup's slivers on the odd frame: under jobs of 16 x 16 and under one job the visited pixels
    differ (the tile-job clamp of the bbox)."""
    mesh = R.hair_soup(np.random.default_rng(8), WO, HO, 300)
    return plain_frame(EYE, 9, w=WO, h=HO, tile=tile, cam_pos=(0.0, 0.0, -3.0)), [M.clip_draw(mesh, mvp=EYE, color=(200, 120, 40, 255))]


def scene_empty():
    view, _ = R.camera()
    return plain_frame(view, 8), []


SCENES = {"demo8": lambda: scene_demo(8), "demo9": lambda: scene_demo(9), "demo10": lambda: scene_demo(10),
          "odd16_8": lambda: scene_demo(8, WO, HO, (16, 16)), "odd16_10": lambda: scene_demo(10, WO, HO, (16, 16)),
          "odd1_8": lambda: scene_demo(8, WO, HO, (WO, HO)), "odd1_9": lambda: scene_demo(9, WO, HO, (WO, HO)),
          "windings": scene_windings, "behind8": scene_behind, "behind10": lambda: scene_behind(10), "prev_behind": scene_prev_behind,
          "coincident8": scene_coincident, "coincident10": lambda: scene_coincident(10), "w_zero": scene_w_zero_line,
          "hair16": lambda: scene_hair((16, 16)), "hair1": lambda: scene_hair((WO, HO)), "empty": scene_empty}


@functools.lru_cache(maxsize=None)
def scene(name):
    return SCENES[name]()


@functools.lru_cache(maxsize=None)
def scene_ref(name):
    """The restatement's planes of a scene, computed once and shared (read only)."""
    frame, draws = scene(name)
    out = ref_render_plain(frame, draws)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def blur_inputs(size=(67, 45)):
    """src: noise over a gradient.  depth (read at either orientation; not symmetric top to bottom): 10 on the left, 20 on
    the right, + 30 in the top third, an empty (FLT_MAX) block and an empty band, and single pixels (spikes: canvas y, x,
    for a plane in screen rows) at depth 5 inside a
    region that moves by 2.7 px (two samples, one pixel to the right and two to the left: both rejected, the pixel is
    copied).  velocity, before the 1.85: normal with sigma 6 (counts from 2 to the clamp at 20, samples that leave the
    canvas), a fifth zero, a block at 0.2 (under the threshold), a block at 1.0 (speed 1.85: the lower clamp), one NaN, one
    +Inf, one -Inf pair.  Read only."""
    w, h = size
    rng = np.random.default_rng(4242)
    yy, xx = np.mgrid[0:h, 0:w]
    src = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    src[..., 0] = (src[..., 0] // 4 + 3 * xx).clip(0, 255)
    src[..., 3] = 255
    depth = np.where(xx < w // 2, F(10), F(20)).astype(F)
    depth[: h // 3] += F(30)
    depth[2:9, w - 12:w - 3] = FLT_MAX
    depth[h - 8:h - 5, :] = FLT_MAX
    vel = rng.normal(0.0, 6.0, (h, w, 2)).astype(F)
    vel[rng.random((h, w)) < 0.2] = 0
    vel[h // 2:h // 2 + 6, 3:12] = (0.2, 0.0)
    vel[h // 2:h // 2 + 6, 14:24] = (1.0, 0.0)
    spikes = [(h // 2 + 10, 8), (h // 2 + 10, 16), (h // 2 + 12, 12)]
    vel[h // 2 + 8:h // 2 + 14, 3:24] = (2.7 / 1.85, 0.0)
    for y, x in spikes:                                   # canvas (y, x): the plane is read at row h - 1 - y
        depth[h - 1 - y, x] = 5
    vel[1, 1] = (np.nan, 1.0)
    vel[1, 3] = (np.inf, 0.0)
    vel[1, 5] = (-np.inf, -np.inf)
    out = dict(src=src, depth=depth, vel=vel, spikes=spikes)
    for v in (src, depth, vel):
        v.setflags(write=False)
    return out


# ---- what fails without the feature, without a GPU -------------------------------------------------------------

ENTRIES = ("shs_rt_render_plain", "shs_canvas_object_blur", "shs_canvas_ping_pong_blur")


def test_library_exports_the_entry_points_and_abi_is_unchanged():
    from shs_gpu import _abi
    L = _abi.lib()
    for name in ENTRIES:
        assert hasattr(L, name), name
    assert L.shs_abi_version() == 1


def test_header_declares_the_entries_and_the_desc_has_its_size(tmp_path):
    """shs_rt_frame is reused as it is; the header declares the three entries with these signatures (compiled, not linked)
    and says where the depth plane's rows are."""
    import shs_gpu
    from shs_gpu import _abi
    decl = tmp_path / "decl.c"
    decl.write_text('#include "shs_gpu.h"\nint (*f)(shs_ctx *, const shs_rt_frame *, const shs_rt_draw *, int32_t) = shs_rt_render_plain;\n'
                    'int (*g)(shs_ctx *, const shs_canvas_object_blur_desc *, const uint8_t *, const float *, const float *, uint8_t *, uint32_t) = '
                    'shs_canvas_object_blur;\nint (*h)(shs_ctx *, int32_t, int32_t, int32_t, uint8_t *, uint32_t) = shs_canvas_ping_pong_blur;\n')
    subprocess.run(["gcc", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", "-o", str(tmp_path / "decl.o"), str(decl)], check=True)
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include "shs_gpu.h"\nint main(void) { printf("%zu %zu %zu %d\\n", sizeof(shs_rt_frame), sizeof(shs_rt_draw), '
                   'sizeof(shs_canvas_object_blur_desc), SHS_CANVAS_MAX_OBJECT_BLUR_SAMPLES); return 0; }\n')
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    sizes = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert sizes == [ctypes.sizeof(_abi.RtFrameC), ctypes.sizeof(_abi.RtDrawC), ctypes.sizeof(_abi.CanvasObjectBlurDescC),
                     _abi.CANVAS_MAX_OBJECT_BLUR_SAMPLES] == [192, 204, 32, 64]
    header = open(os.path.join(ROOT, "include", "shs_gpu.h")).read()
    assert "THE DEPTH PLANE IS IN SCREEN ROWS" in header and "py * W + px" in header
    assert shs_gpu.Context.FX_DEFAULTS["object_blur"] == dict(multiplier=1.85, velocity_scale=1.0, min_vel2=0.25, max_samples=20,
                                                              depth_eps=0.15, depth_rows=1)


# ---- the numpy witnesses ----------------------------------------------------------------------------------------

RASTER_SWAPS = ("ambient_0.35", "canvas_depth_rows", "view_z_for_10", "frag_velocity")


def np_render_plain(frame, draws, swap=None):
    """The whole pass in float32 numpy: per tile job and triangle, the pixels of the clamped bbox at once.  depth is indexed
    [py, px] (screen rows), every other plane [H - 1 - py, px].  swap: one neighbouring rule in place of this pass's."""
    Wd, Hd = frame.width, frame.height
    tw, th = min(frame.ref_tile[0], Wd), min(frame.ref_tile[1], Hd)
    sh = frame.shading
    depth = np.full((Hd, Wd), FLT_MAX, F)
    ids = np.full((Hd, Wd), -1, np.int32)
    vel = np.zeros((Hd, Wd, 2), F)
    pq = np.zeros((Hd, Wd, 4), F)
    kept = 0
    ambient = F(0.35) if swap == "ambient_0.35" else F(0.15)
    L = M._norm3(-np.asarray(frame.light_dir_world, F))
    cam = np.asarray(frame.camera_pos, F)

    def screen(p):
        return ((p[..., 0] / p[..., 3] + F(1)) * F(0.5)) * F(Wd - 1), ((F(1) - p[..., 1] / p[..., 3]) * F(0.5)) * F(Hd - 1)

    with np.errstate(all="ignore"):
        vs, base = [], 0
        for d in draws:
            pos = np.asarray(d.mesh.positions, F).reshape(-1, 3, 3)
            nrm = np.asarray(d.mesh.normals, F).reshape(-1, 3, 3)
            inv = SK.np_inverse(d.model)
            n3 = [inv[r * 4 + c] for c in range(3) for r in range(3)]          # mat3(transpose(inverse(model))), column-major
            n = np.stack([n3[0 + r] * nrm[..., 0] + n3[3 + r] * nrm[..., 1] + n3[6 + r] * nrm[..., 2] for r in range(3)], -1)
            clip = M._m4(d.mvp, pos)
            sx, sy = screen(clip)
            if sh == 10 and swap != "view_z_for_10":
                zc = clip[..., 2] / clip[..., 3]                                # clip_to_screen's z
            else:
                zc = M._m4(R._mul(frame.view, d.model), pos)[..., 2]             # view_z
            vs.append(dict(clip=clip, prev=M._m4(d.prev_mvp, pos), world=M._m4(d.model, pos)[..., :3], n=M._norm3(n), zc=zc, sx=sx, sy=sy,
                           base=base, col=np.array(d.base_color[:3], F) / F(255)))
            base += pos.shape[0]
        first = True
        for ty in range((Hd + th - 1) // th):
            for tx in range((Wd + tw - 1) // tw):
                tminx, tminy = F(tx * tw), F(ty * th)
                tmaxx, tmaxy = F(min((tx + 1) * tw, Wd) - 1), F(min((ty + 1) * th, Hd) - 1)
                for v in vs:
                    for k in range(v["sx"].shape[0]):
                        sx, sy = v["sx"][k], v["sy"][k]
                        bx0, by0, bx1, by1 = tmaxx, tmaxy, tminx, tminy
                        for i in range(3):
                            bx0, by0 = M._gmax(tminx, M._gmin(bx0, sx[i])), M._gmax(tminy, M._gmin(by0, sy[i]))
                            bx1, by1 = M._gmin(tmaxx, M._gmax(bx1, sx[i])), M._gmin(tmaxy, M._gmax(by1, sy[i]))
                        v0x, v0y, v1x, v1y = sx[1] - sx[0], sy[1] - sy[0], sx[2] - sx[0], sy[2] - sy[0]
                        area = v0x * v1y - v0y * v1x
                        culled = bool(area <= 0)
                        if first and not culled:
                            kept += 1
                        if bx0 > bx1 or by0 > by1 or culled:
                            continue
                        d00, d01, d11 = v0x * v0x + v0y * v0y, v0x * v1x + v0y * v1y, v1x * v1x + v1y * v1y
                        den = d00 * d11 - d01 * d01
                        if abs(float(den)) < 1e-5:
                            continue
                        xs, ys = np.arange(int(bx0), int(bx1) + 1), np.arange(int(by0), int(by1) + 1)
                        vpx = ((xs.astype(F) + F(0.5)) - sx[0])[None, :]
                        vpy = ((ys.astype(F) + F(0.5)) - sy[0])[:, None]
                        d20, d21 = vpx * v0x + vpy * v0y, vpx * v1x + vpy * v1y
                        bv = (d11 * d20 - d01 * d21) / den
                        bw = (d00 * d21 - d01 * d20) / den
                        bu = F(1) - bv - bw
                        zc = v["zc"][k]
                        z = (bu * zc[0] + bv * zc[1]) + bw * zc[2]
                        cy = Hd - 1 - ys
                        drow = cy if swap == "canvas_depth_rows" else ys         # the ZBuffer's row: the screen row
                        win = ~((bu < 0) | (bv < 0) | (bw < 0)) & (z < depth[np.ix_(drow, xs)])
                        if not win.any():
                            continue
                        iy, ix = np.nonzero(win)
                        oy, ox = cy[iy], xs[ix]
                        u, b, w = bu[iy, ix], bv[iy, ix], bw[iy, ix]
                        depth[drow[iy], ox] = z[iy, ix]
                        N = M._norm3(M._norm3(M._mix(u, b, w, *v["n"][k])))
                        world = M._mix(u, b, w, *v["world"][k])
                        if sh == 8:
                            pc, pp = M._mix(u, b, w, *v["clip"][k]), M._mix(u, b, w, *v["prev"][k])
                            if swap == "frag_velocity":                          # multi :583-591 under max_velocity_px
                                csx, csy = screen(pc)
                                psx, psy = screen(pp)
                                vx, vy = csx - psx, -(csy - psy)
                                ln = np.sqrt(vx * vx + vy * vy)
                                cl = (ln > F(frame.max_velocity_px)) & (ln > F(0.0001))
                                s = np.where(cl, F(frame.max_velocity_px) / ln, F(1))
                                vx, vy = np.where(cl, vx * s, vx), np.where(cl, vy * s, vy)
                            else:                                                # per :170-174
                                vx = ((pc[:, 0] / pc[:, 3] - pp[:, 0] / pp[:, 3]) * F(0.5)) * F(Wd)
                                vy = ((pc[:, 1] / pc[:, 3] - pp[:, 1] / pp[:, 3]) * F(0.5)) * F(Hd)
                            vel[oy, ox, 0], vel[oy, ox, 1] = vx, vy
                        V = M._norm3(cam - world)
                        dot = lambda a, c: (a[..., 0] * c[..., 0] + a[..., 1] * c[..., 1]) + a[..., 2] * c[..., 2]   # noqa: E731
                        ndl = dot(N, L)
                        diffuse = np.where(ndl < 0, F(0), ndl)
                        ndh = dot(N, M._norm3(L + V))
                        ndh = np.where(ndh < 0, F(0), ndh)
                        lit = (ambient + diffuse) + F(0.5) * M._powf(ndh, 64.0)
                        res = lit[:, None] * v["col"][None, :]
                        res = np.where(res < 0, F(0), res)
                        res = np.where(F(1) < res, F(1), res)
                        pq[oy, ox, :3] = res * F(255)
                        pq[oy, ox, 3] = 1
                        ids[oy, ox] = 2 * (v["base"] + k)
                first = False
        color = np.empty((Hd, Wd, 4), np.uint8)
        color[...] = np.array(frame.clear_color, np.uint8)
        shown = ids >= 0
        color[shown, :3] = np.nan_to_num(pq[shown, :3], nan=0.0).astype(np.int32).astype(np.uint8)   # x86: (uint8_t)NaN is 0
        color[shown, 3] = 255
    return dict(depth=depth, tri_id=ids, velocity=vel, prequant=pq, color=color, kept=kept)


def _int_x86(f):
    """(int)f as cvttss2si gives it: INT_MIN for a NaN or a value outside int's range."""
    f = np.asarray(f, F)
    ok = np.isfinite(f) & (f >= F(-2147483648.0)) & (f < F(2147483648.0))
    return np.where(ok, np.trunc(np.where(ok, f, 0)).astype(np.int64), INT_MIN)


BLUR_SWAPS = ("kernel_0_1", "no_depth_rejection")


def np_object_blur(src, depth, vel, swap=None, **over):
    """post_process_motion_blur (per :461-552) in float32 numpy, every pixel at once, one sample index after the other ->
    dict(out, samples [h, w] (0: copied under the threshold), kept, outside: per pixel the samples that survived and those
    that left the canvas)."""
    p = blur_params(**over)
    h, w = depth.shape
    yy, xx = np.mgrid[0:h, 0:w]
    with np.errstate(all="ignore"):
        k = F(p["multiplier"]) * F(p["velocity_scale"])
        vx, vy = np.asarray(vel[..., 0], F) * k, np.asarray(vel[..., 1], F) * k
        vv = vx * vx + vy * vy
        small = vv < F(p["min_vel2"])
        samples = np.clip(_int_x86(np.sqrt(vv)), 2, p["max_samples"])

        def zat(x, y):
            return depth[(h - 1 - y) if p["depth_rows"] else y, x]
        z0 = zat(xx, yy)
        acc = np.zeros((h, w, 3), F)
        wsum = np.zeros((h, w), F)
        outside = np.zeros((h, w), np.int32)
        for s in range(p["max_samples"]):
            act = ~small & (s < samples)
            t = F(s) / (samples - 1).astype(F)
            o = t if swap == "kernel_0_1" else t - F(0.5)
            sx, sy = _int_x86(xx.astype(F) - vx * o), _int_x86(yy.astype(F) - vy * o)
            inb = (sx >= 0) & (sx < w) & (sy >= 0) & (sy < h)
            outside += act & ~inb
            cx, cy = np.where(inb, sx, 0), np.where(inb, sy, 0)
            take = act & inb
            if swap != "no_depth_rejection":
                take &= ~(np.abs(zat(cx, cy) - z0) > F(p["depth_eps"]))
            acc += np.where(take[..., None], src[cy, cx, :3].astype(F), F(0))
            wsum += take.astype(F)
        mean = acc / wsum[..., None]
        v = np.where(F(0) < mean, mean, F(0))
        v = np.where(v < F(255), v, F(255))
        out = np.array(src, np.uint8, copy=True)
        g = ~small & (wsum > 0)
        out[g, :3] = v[g].astype(np.int32).astype(np.uint8)
        out[g, 3] = 255
    return dict(out=out, samples=np.where(small, 0, samples), kept=wsum.astype(np.int32), outside=outside)


def _bits(a):
    return P.canonical_bits(a)


def assert_witness(ref, wit, label):
    assert np.array_equal(ref["tri_id"], wit["tri_id"]), f"{label}: ids"
    for k in ("depth", "velocity"):
        bad = np.argwhere(_bits(ref[k]) != _bits(wit[k]))
        assert bad.size == 0, f"{label}: {len(bad)} {k} words differ, first {bad[:3].tolist()}"
    a, b = ref["prequant"], wit["prequant"]
    assert np.array_equal(np.isnan(a), np.isnan(b)), f"{label}: NaN colour floats on one side only"
    assert np.array_equal(_bits(a[..., 3]), _bits(b[..., 3]))
    helpers.assert_color_parity(wit["color"], ref["color"], np.nan_to_num(b), np.nan_to_num(a))
    assert ref["counters"]["sub_tris"] == wit["kept"] and ref["counters"]["polys3"] == ref["counters"]["polys4"] == 0


@pytest.mark.parametrize("name", list(SCENES))
def test_restatement_equals_numpy_witness(name):
    frame, draws = scene(name)
    assert_witness(scene_ref(name), np_render_plain(frame, draws), name)


@pytest.mark.parametrize("over", [{}, dict(depth_rows=0), dict(velocity_scale=4.0, max_samples=64), dict(velocity_scale=0.25, max_samples=2),
                                  dict(multiplier=1.0, min_vel2=0.0, depth_eps=0.0)],
                         ids=["demo", "canvas_rows", "fast_64", "slow_2", "no_threshold"])
def test_blur_restatement_equals_numpy_witness(over):
    inp = blur_inputs()
    ref, gathered = ref_object_blur(inp["src"], inp["depth"], inp["vel"], **over)
    wit = np_object_blur(inp["src"], inp["depth"], inp["vel"], **over)
    assert np.array_equal(ref, wit["out"]), f"{int((ref != wit['out']).any(-1).sum())} pixels differ"
    assert gathered == int(((wit["samples"] > 0) & (wit["kept"] > 0)).sum())


# ---- known answers ------------------------------------------------------------------------------------------------

def _filling_triangle(mvp, prev):
    """Screen corners A (-10, -10), B (100, -10), C (-10, 100) on a 41 x 41 frame (screen = (ndc + 1) * 20, y down): every
    pixel centre lies inside (x + y <= 81 < 90).  clip z = 0.25 / 0.5 / 0.75 at A / B / C."""
    import shs_gpu
    sx = lambda px: px / 20.0 - 1.0      # noqa: E731
    sy = lambda py: 1.0 - py / 20.0      # noqa: E731
    tri = [sx(-10), sy(-10), 0.25, sx(100), sy(-10), 0.5, sx(-10), sy(100), 0.75]
    mesh = R.SoupMesh(np.array([tri], F), np.array([[0, 0, -1] * 3], F))
    return [shs_gpu.RtDraw(mesh, EYE, np.asarray(mvp, F), np.asarray(prev, F), (101, 47, 7, 255))]


def test_filling_triangle_known_answers():
    """At screen pixel (15, 15), centre (15.5, 15.5): v = w = 25.5 / 110, depth = 0.25 + 0.75 * 25.5 / 110 = 0.4238636; at
    screen pixel (15, 25): v = 25.5 / 110, w = 35.5 / 110, depth = 0.25 + 0.25 * 25.5 / 110 + 0.5 * 35.5 / 110 = 0.4693182.
    The depth plane holds them at rows 15 and 25 (screen rows); ids and colour at rows 25 and 15 (canvas rows: 40 - py).
    Shading 8, prev_mvp = mvp shifted by -0.1 in clip x and +0.05 in clip y at w = 1: velocity = (0.1 * 0.5 * 41, -0.05 *
    0.5 * 41) = (2.05, -1.025) at every pixel.  N . L = N . H = 1: lit = 0.15 + 1 + 0.5 = 1.65; colour (101, 47, 7) ->
    166.65, 77.55, 11.55 -> (166, 77, 11).  Shading 10 with mvp = diag(2, 2, 1, 2): the same screen, depth = clip z / 2."""
    prev = EYE.copy()
    prev[12], prev[13] = -0.1, 0.05
    frame = plain_frame(EYE, 8, w=41, h=41, tile=(41, 41), cam_pos=(0.0, 0.0, -1e6), light_dir=(0.0, 0.0, 1.0))
    out = ref_render_plain(frame, _filling_triangle(EYE, prev))
    assert (out["tri_id"] == 0).all() and out["counters"] == {"input_tris": 1, "polys3": 0, "polys4": 0, "sub_tris": 1}
    assert abs(out["depth"][15, 15] - (0.25 + 0.75 * 25.5 / 110)) < 1e-6
    assert abs(out["depth"][25, 15] - (0.25 + 0.25 * 25.5 / 110 + 0.5 * 35.5 / 110)) < 1e-6
    assert abs(out["depth"][25, 15] - out["depth"][15, 15]) > 0.04            # a plane in canvas rows would swap the two
    assert np.abs(out["velocity"] - np.array([2.05, -1.025], F)).max() < 1e-5
    assert tuple(out["color"][40 - 15, 15]) == (166, 77, 11, 255) and (out["prequant"][..., 3] == 1).all()
    # shading 9: the same depth, no velocity
    out9 = ref_render_plain(dataclasses.replace(frame, shading=9), _filling_triangle(EYE, prev))
    assert np.array_equal(out9["depth"], out["depth"]) and not out9["velocity"].any() and np.array_equal(out9["color"], out["color"])
    # shading 10: clip z / clip w, whatever the view matrix says
    half = EYE.copy()
    half[0] = half[5] = half[15] = 2.0
    view = EYE.copy()
    view[10], view[14] = 3.0, 7.0
    out10 = ref_render_plain(dataclasses.replace(frame, shading=10, view=view), _filling_triangle(half, half))
    assert np.abs(out10["depth"] - out["depth"] / 2).max() < 1e-6 and not out10["velocity"].any()
    out9v = ref_render_plain(dataclasses.replace(frame, shading=9, view=view), _filling_triangle(half, half))
    assert np.abs(out9v["depth"] - (out["depth"] * 3 + 7)).max() < 1e-5
    # the other winding shows nothing
    import shs_gpu
    d = _filling_triangle(EYE, prev)[0]
    back = [shs_gpu.RtDraw(R.SoupMesh(d.mesh.positions.reshape(1, 3, 3)[:, [0, 2, 1]].reshape(1, 9), d.mesh.normals), EYE, EYE, EYE)]
    out = ref_render_plain(frame, back)
    assert (out["tri_id"] == -1).all() and out["counters"]["sub_tris"] == 0 and (out["depth"] == FLT_MAX).all()


def test_blur_pixel_known_answers():
    """A 9 x 3 canvas, red = 10 x, depth 1, multiplier and scale 1, the pixel (4, 1) moving by v = (4, 0): four samples at
    offsets -1/2, -1/6, 1/6, 1/2 of v: x = (int)6, (int)4.67, (int)3.33, (int)2 = 6, 4, 3, 2 -> (60 + 40 + 30 + 20) / 4 =
    37.5 -> 37.  With the depth at x = 6 moved to 5 that sample is rejected: (40 + 30 + 20) / 3 = 30.  With every depth but
    the pixel's own moved, only x = 4 survives: 40.  v = (0.4, 0): 0.16 < 0.25, copied.  v = (0, -30): 20 samples, rows
    (int)(1 + 30 o) for o from -0.5: -14 .. 16, of which rows 0, 1, 2 are inside (o = -1/38, 1/38, 3/38 -> 0.21, 1.79, 3.4:
    rows 0 and 1 only): the mean of two equal reds."""
    src = np.zeros((3, 9, 4), np.uint8)
    src[..., 0] = 10 * np.arange(9)
    src[..., 3] = 255
    depth = np.ones((3, 9), F)
    vel = np.zeros((3, 9, 2), F)
    vel[1, 4] = (4, 0)
    kw = dict(multiplier=1.0, velocity_scale=1.0, depth_rows=0)
    out, n = ref_object_blur(src, depth, vel, **kw)
    assert n == 1 and tuple(out[1, 4]) == (37, 0, 0, 255) and np.array_equal(np.delete(out.reshape(-1, 4), 13, 0), np.delete(src.reshape(-1, 4), 13, 0))
    d2 = depth.copy()
    d2[1, 6] = 5
    assert tuple(ref_object_blur(src, d2, vel, **kw)[0][1, 4]) == (30, 0, 0, 255)
    d3 = np.full((3, 9), F(7))
    d3[1, 4] = 1
    assert tuple(ref_object_blur(src, d3, vel, **kw)[0][1, 4]) == (40, 0, 0, 255)
    # screen rows: the pixel's depth is read at row 3 - 1 - 1 = 1 again, its neighbours' too: the same answer
    assert tuple(ref_object_blur(src, d2, vel, **dict(kw, depth_rows=1))[0][1, 4]) == (30, 0, 0, 255)
    vel[1, 4] = (0.4, 0)
    out, n = ref_object_blur(src, depth, vel, **kw)
    assert n == 0 and np.array_equal(out, src)
    vel[1, 4] = (0, -30)
    out, n = ref_object_blur(src, depth, vel, **kw)
    assert n == 1 and tuple(out[1, 4]) == (40, 0, 0, 255)
    w = np_object_blur(src, depth, vel, **kw)
    assert w["samples"][1, 4] == 20 and w["kept"][1, 4] == 2 and w["outside"][1, 4] == 18


# ---- the scenes and inputs show what they are there for -------------------------------------------------------------

def test_scenes_cover_what_the_gpu_tests_need():
    for name in ("demo8", "odd16_8", "odd1_8"):
        out = scene_ref(name)
        frame, draws = scene(name)
        shown = out["tri_id"] >= 0
        per = draws[0].mesh.positions.shape[0]
        which = out["tri_id"] // 2 // per
        ln = np.hypot(out["velocity"][..., 0], out["velocity"][..., 1])
        assert out["counters"]["input_tris"] == 2 * per + 2 and 2 * out["counters"]["input_tris"] > 256
        assert 0 < out["counters"]["sub_tris"] < out["counters"]["input_tris"]                    # both windings
        assert set(np.unique(which[shown])) == {0, 1, 2} and (out["tri_id"][shown] % 2 == 0).all()
        assert (ln[shown & (which == 1)] == 0).all() and (shown & (which == 1)).sum() > 50      # prev_mvp == mvp: exactly zero
        assert (ln[shown & (which == 0)] > 1).sum() > 50 and (ln[shown & (which == 2)] > 1).sum() > 100
        assert not out["velocity"][~shown].any()
        # asymmetric top to bottom: the depth plane is not its own mirror image, and it is the ids' plane turned over
        empty = out["depth"] == FLT_MAX
        assert np.array_equal(empty[::-1], ~shown) and not np.array_equal(empty, ~shown)
    for name in ("demo9", "demo10"):
        out = scene_ref(name)
        assert not out["velocity"].any() and np.array_equal(out["tri_id"] >= 0, scene_ref("demo8")["tri_id"] >= 0)
    assert np.array_equal(scene_ref("demo9")["depth"], scene_ref("demo8")["depth"])
    d10 = scene_ref("demo10")["depth"]
    assert (d10[d10 != FLT_MAX] < 1).all() and (d10[d10 != FLT_MAX] > 0.8).all()                    # clip z / w of a perspective camera

    out = scene_ref("windings")
    assert set(np.unique(out["tri_id"])) == {-1, 0, 2} and out["counters"]["sub_tris"] == 2

    out = scene_ref("behind8")
    ids, v = out["tri_id"], out["velocity"]
    assert set(np.unique(ids)) == {-1, 0, 6, 8} and (ids == 0).sum() > 300
    vx = np.nan_to_num(v[ids == 0][:, 0])
    assert (vx > 20).any() and (vx < -20).any(), "the interpolated w does not change sign inside the drawn triangle"
    assert np.isfinite(v[ids == 8]).all()
    out = scene_ref("w_zero")
    v = out["velocity"]
    assert (out["tri_id"] == 0).sum() > 1500 and np.isnan(v[HO - 1 - 6, 18]).all() and np.isnan(v[HO - 1 - 6, 55]).all()
    fin = v[(out["tri_id"] == 0) & np.isfinite(v).all(-1)]
    assert len(fin) > 1500 and not fin.any()                           # prev_mvp == mvp elsewhere: exactly zero

    out = scene_ref("prev_behind")
    v = out["velocity"]
    assert (~np.isfinite(v[out["tri_id"] >= 4])).any() and np.isfinite(v[(out["tri_id"] >= 0) & (out["tri_id"] < 4)]).any()
    assert np.abs(v[np.isfinite(v)]).max() > 40.001                                                # nothing clamps it

    for name in ("coincident8", "coincident10"):
        out = scene_ref(name)
        assert set(np.unique(out["tri_id"])) == {-1, 0} and ((out["flags"] & PX_ZTIE) != 0).sum() > 500 and out["counters"]["sub_tris"] == 2

    a, b = scene_ref("hair16"), scene_ref("hair1")
    assert (a["depth"].view(np.uint32) != b["depth"].view(np.uint32)).sum() >= 10                  # the tile-job clamp changes the image

    out = scene_ref("empty")
    assert (out["tri_id"] == -1).all() and (out["depth"] == FLT_MAX).all() and not out["velocity"].any()
    assert (out["color"] == np.array(scene("empty")[0].clear_color, np.uint8)).all() and out["counters"]["input_tris"] == 0


def test_blur_inputs_cover_what_the_gpu_tests_need():
    inp = blur_inputs()
    w = np_object_blur(inp["src"], inp["depth"], inp["vel"])
    s, kept, outside = w["samples"], w["kept"], w["outside"]
    assert (s == 0).sum() > 400 and (s == 2).sum() > 100 and (s == 20).sum() > 100 and ((s > 2) & (s < 20)).sum() > 500
    assert (outside > 0).sum() > 200
    for y, x in inp["spikes"]:
        assert s[y, x] == 2 and kept[y, x] == 0 and outside[y, x] == 0, "the spike's two samples are not both depth-rejected"
        assert np.array_equal(w["out"][y, x], inp["src"][y, x])
    # empty depth on one side of a comparison (rejected) and on both (kept: FLT_MAX - FLT_MAX = 0)
    empty = (inp["depth"] == FLT_MAX)[::-1]                     # in canvas rows
    assert ((s > 2) & empty & (kept > 0)).sum() > 20 and ((s > 2) & empty & (kept + outside < s)).sum() > 20
    # the NaN and Inf velocities: two samples, both outside, copied
    for x in (1, 3, 5):
        assert s[1, x] == 2 and outside[1, x] == 2 and np.array_equal(w["out"][1, x], inp["src"][1, x])
    assert (w["out"] != inp["src"]).any(-1).sum() > 1000


@pytest.mark.parametrize("swap,name", [("ambient_0.35", "demo9"), ("canvas_depth_rows", "demo8"), ("view_z_for_10", "demo10"),
                                       ("frag_velocity", "demo8")])
def test_rule_swaps_change_pixels(swap, name):
    frame, draws = scene(name)
    ref = scene_ref(name)
    wit = np_render_plain(frame, draws, swap)
    moved = (ref["tri_id"] != wit["tri_id"]) | (_bits(ref["velocity"]) != _bits(wit["velocity"])).any(-1) | (_bits(ref["depth"]) != _bits(wit["depth"]))
    with np.errstate(invalid="ignore"):
        moved |= (np.nan_to_num(np.abs(ref["prequant"][..., :3] - wit["prequant"][..., :3]), nan=0.0) > BAR).any(-1)
    assert moved.sum() > 200, f"{swap} on {name}: {int(moved.sum())} pixels changed"


@pytest.mark.parametrize("swap", BLUR_SWAPS + ("depth_rows",))
def test_blur_rule_swaps_change_pixels(swap):
    inp = blur_inputs()
    ref, _ = ref_object_blur(inp["src"], inp["depth"], inp["vel"])
    if swap == "depth_rows":
        other = np_object_blur(inp["src"], inp["depth"], inp["vel"], depth_rows=0)["out"]
    else:
        other = np_object_blur(inp["src"], inp["depth"], inp["vel"], swap=swap)["out"]
    assert (ref != other).any(-1).sum() > 100, f"{swap}: {int((ref != other).any(-1).sum())} pixels changed"


def test_depth_orientation_shows_in_the_dof_and_blur_results():
    """The demo scene is asymmetric top to bottom: the DoF composite over the screen-row depth plane (what the demo
    computes) differs from the one over that plane turned the right way up, the autofocus depth too; and the blur that reads
    screen rows differs from one told the plane is in canvas rows."""
    from oracle import oracle
    out = scene_ref("demo9")
    kw = dict(iterations=3, radius=6, focus=None, range_=24.0, max_blur=0.6)
    as_demo = oracle.canvas_dof(out["color"], out["depth"], **kw)
    upright = oracle.canvas_dof(out["color"], out["depth"][::-1], **kw)
    assert (as_demo[0] != upright[0]).any(-1).sum() > 200
    out = scene_ref("demo8")
    a = ref_object_blur(out["color"], out["depth"], out["velocity"], depth_rows=1)[0]
    b = ref_object_blur(out["color"], out["depth"], out["velocity"], depth_rows=0)[0]
    assert (a != b).any(-1).sum() > 50 and (a != out["color"]).any(-1).sum() > 200
