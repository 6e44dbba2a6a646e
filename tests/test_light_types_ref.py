"""CPU tests of the typed local lights: the C restatement of the four ILightModel::sample functions
(tests/light_types_ref/ref_light_models.c, the GPU tests' reference), shs_light_pack_culling and the new
ABI surface.

The reference library is the frozen oracle with its rasteriser's per-light call renamed to the
restatement (tests/light_types_ref/Makefile).  Known answers are computed here by hand in float32 numpy
from lighting/light_runtime.hpp's lines (cosf / powf through libm, as the reference's std::cos / std::pow)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REF_DIR = os.path.join(HERE, "light_types_ref")
REF_LIB = os.path.join(REF_DIR, "_build", "libshs_light_types_ref.so")
F = np.float32
_P = ctypes.c_void_p
_ref = None
_libm = ctypes.CDLL("libm.so.6")
for _n in ("cosf", "powf"):
    getattr(_libm, _n).restype = ctypes.c_float
_libm.cosf.argtypes = [ctypes.c_float]
_libm.powf.argtypes = [ctypes.c_float, ctypes.c_float]


def ref_lib():
    """libshs_light_types_ref.so, built by make as tests/test_abi_c.py builds its hosts."""
    global _ref
    if _ref is None:
        subprocess.run(["make", "-s", "-C", REF_DIR], check=True)
        L = ctypes.CDLL(REF_LIB)
        L.ref_light_sample.restype = None
        L.ref_light_sample.argtypes = [_P] * 5
        L.ref_set_light_props.restype = None
        L.ref_set_light_props.argtypes = [_P, _P, ctypes.c_int]
        L.ref_typed_light_accumulate.restype = None
        L.ref_typed_light_accumulate.argtypes = [_P] * 6
        L.ora_point_light_accumulate.restype = None
        L.ora_point_light_accumulate.argtypes = [_P] * 6
        L.ref_light_misses.restype = ctypes.c_int
        L.ref_sizeof.restype = ctypes.c_int
        L.ref_sizeof.argtypes = [ctypes.c_int]
        _ref = L
    return _ref


def typed_reference(monkeypatch, oracle_mod, frame, draws, cull_recs, props, cull, lists):
    """oracle.forward_plus over the reference library: `draws` with the typed program run as program-5
    draws (which the frozen rasteriser knows), every listed light through ref_typed_light_accumulate with
    props[i] for record i of cull_recs.  Both arrays must be C-contiguous (the registered base pointer is
    the one the C code sees)."""
    from shs_gpu.lib_path import LIGHT_DTYPE, LIGHT_PROPS_DTYPE, PROGRAM_FORWARD_PLUS, PROGRAM_FORWARD_PLUS_TYPED
    assert cull_recs.dtype == LIGHT_DTYPE and cull_recs.flags.c_contiguous
    assert props.dtype == LIGHT_PROPS_DTYPE and props.flags.c_contiguous and len(props) == len(cull_recs)
    L = ref_lib()
    ref_draws = [type(d)(**{**d.__dict__, "program": PROGRAM_FORWARD_PLUS}) if d.program == PROGRAM_FORWARD_PLUS_TYPED else d
                 for d in draws]
    L.ref_set_light_props(cull_recs.ctypes.data, props.ctypes.data, len(props))
    with monkeypatch.context() as m:
        m.setattr(oracle_mod, "_lib", L)
        out = oracle_mod.forward_plus(frame, ref_draws, cull_recs, cull, lists)
    assert L.ref_light_misses() == 0, "the reference saw a light record outside the registered table"
    return out


def sample(p, world, n, v):
    """ILightModel::sample of one LIGHT_PROPS_DTYPE record -> (diffuse[3], specular[3])."""
    rec = np.ascontiguousarray(np.asarray(p).reshape(1))
    a = [np.ascontiguousarray(x, dtype=F).reshape(3) for x in (world, n, v)]
    out = np.full(6, 7.0, F)
    ref_lib().ref_light_sample(rec.ctypes.data, a[0].ctypes.data, a[1].ctypes.data, a[2].ctypes.data, out.ctypes.data)
    return out[:3].copy(), out[3:].copy()


# ---- float32 hand computation of the cited lines ------------------------------------------------
def _dot(a, b):
    return F(F(F(a[0] * b[0]) + F(a[1] * b[1])) + F(a[2] * b[2]))


def _v(*x):
    return np.array(x, F)


def _normalize_or(v, fb):
    l2 = _dot(v, v)
    return fb if l2 <= F(1e-10) else (v * F(F(1.0) / np.sqrt(l2))).astype(F)


def _atten(p, dist):   # eval_distance_attenuation (:182-210)
    rng = max(F(p["range"]), F(0.001))
    if dist >= rng:
        return F(0.0)
    norm = min(max(F(F(1.0) - F(dist / rng)), F(0.0)), F(1.0))
    m = int(p["attenuation_model"])
    if m == 0:
        fall = norm
    elif m == 1:
        fall = F(F(norm * norm) * F(F(3.0) - F(F(2.0) * norm)))
    else:
        inv = F(F(1.0) / max(F(dist * dist), F(p["attenuation_bias"])))
        fall = F(min(F(1.0), F(inv * F(rng * rng))) * F(norm * norm))
    fall = F(_libm.powf(max(fall, F(0.0)), max(F(p["attenuation_power"]), F(0.001))))
    if p["attenuation_cutoff"] > 0 and fall < F(p["attenuation_cutoff"]):
        return F(0.0)
    return max(fall, F(0.0))


def _tail(p, L, dist, shaping, spec_power, spec_scale, n, v):   # eval_local_light_brdf (:212-237)
    z = np.zeros(3, F)
    ndotl = max(_dot(n, L), F(0.0))
    if ndotl <= 0:
        return z, z
    att = F(_atten(p, dist) * max(F(shaping), F(0.0)))
    if att <= 0:
        return z, z
    rad = ((np.maximum(p["color"].astype(F), F(0.0)) * max(F(p["intensity"]), F(0.0))).astype(F) * att).astype(F)
    H = _normalize_or((L + v).astype(F), L)
    spec = F(F(spec_scale) * F(_libm.powf(max(_dot(n, H), F(0.0)), F(spec_power))))
    return (rad * ndotl).astype(F), (rad * spec).astype(F)


def _from_emit(p, emit, world):
    tl = (emit - world).astype(F)
    dist = np.sqrt(_dot(tl, tl))
    return (tl / dist).astype(F), dist


def _bits(a):
    return np.asarray(a, F).view(np.uint32)


def _props(light_type, **kw):
    from shs_gpu.lib_path import light_props
    p = light_props(1, light_type)
    for k, val in kw.items():
        p[k] = val
    return p[0]


UP = _v(0.0, 1.0, 0.0)
VIEW = _normalize_or(_v(0.3, 0.8, -0.2), UP)


def _same(got, want):
    assert np.array_equal(_bits(got[0]), _bits(want[0])) and np.array_equal(_bits(got[1]), _bits(want[1])), (got, want)


def _zero(got):
    assert not np.any(_bits(got[0])) and not np.any(_bits(got[1])), got


# ---- the restatement ---------------------------------------------------------------------------
def test_point_restriction_equals_frozen_oracle_bitwise():
    """10,000 random (world, N, V, light) draws over the three attenuation models: the restatement on
    Point lights and the frozen ora_point_light_accumulate (both symbols of the reference library) give
    the same `lit` bits."""
    from shs_gpu.lib_path import make_point_props, pack_culling
    L = ref_lib()
    rng = np.random.default_rng(0x7E57)
    n = 10000
    props = make_point_props(rng.uniform(-4, 4, (n, 3)), rng.uniform(1.0, 9.0, n), rng.uniform(-0.1, 1.0, (n, 3)),
                             rng.uniform(0.2, 2.0, n))
    props["attenuation_model"] = np.arange(n) % 3
    props["attenuation_power"] = rng.choice([1.0, 0.5, 2.5], n)
    props["attenuation_bias"] = rng.choice([0.05, 0.5], n)
    props["attenuation_cutoff"] = rng.choice([0.0, 0.1], n)
    recs = pack_culling(props)
    world = (props["position_ws"] + rng.normal(size=(n, 3)) * rng.uniform(0.2, 4.0, (n, 1))).astype(F)
    nrm = rng.normal(size=(n, 3))
    nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(F)
    view = rng.normal(size=(n, 3))
    view = (view / np.linalg.norm(view, axis=1, keepdims=True)).astype(F)
    base = rng.uniform(0.1, 1.0, (n, 3)).astype(F)
    start = rng.uniform(0.0, 0.5, (n, 3)).astype(F)
    a, b = start.copy(), start.copy()
    L.ref_set_light_props(recs.ctypes.data, props.ctypes.data, n)
    for i in range(n):
        args = (recs[i:].ctypes.data, world[i:].ctypes.data, nrm[i:].ctypes.data, view[i:].ctypes.data, base[i:].ctypes.data)
        L.ora_point_light_accumulate(*args, a[i:].ctypes.data)
        L.ref_typed_light_accumulate(*args, b[i:].ctypes.data)
    assert L.ref_light_misses() == 0
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    lit = (a != start).any(axis=1)
    for m in range(3):   # every model lit a good share of its draws
        assert int(lit[props["attenuation_model"] == m].sum()) > 300, m


def test_spot_on_axis_inside_inner_cone():
    p = _props(2, position_ws=(0.0, 3.0, 0.0), direction_ws=(0.0, -1.0, 0.0), range=8.0, color=(0.9, 0.5, 0.3), intensity=1.5)
    world = _v(0.0, 0.0, 0.0)
    L, dist = _from_emit(p, p["position_ws"], world)
    inner = min(max(F(p["inner_angle_rad"]), F(0.02)), F(F(np.pi / 2) - F(0.02)))
    outer = min(max(max(F(inner + F(0.005)), F(p["outer_angle_rad"])), F(inner + F(0.005))), F(F(np.pi / 2) - F(0.005)))
    ci, co = F(_libm.cosf(inner)), F(_libm.cosf(outer))
    t = min(max(F(F(_dot(-L, _v(0.0, -1.0, 0.0)) - co) / max(F(ci - co), F(1e-5))), F(0.0)), F(1.0))
    shaping = F(F(t * t) * F(F(3.0) - F(F(2.0) * t)))
    assert shaping == F(1.0)   # inside the inner cone: exactly 1
    want = _tail(p, L, dist, 1.0, 34.0, 0.32, UP, VIEW)
    got = sample(p, world, UP, VIEW)
    assert got[0].min() > 0 and got[1].min() > 0
    _same(got, want)


def test_spot_outside_outer_cone_is_zero():
    p = _props(2, position_ws=(0.0, 3.0, 0.0), direction_ws=(0.0, -1.0, 0.0), range=8.0)
    _zero(sample(p, _v(2.5, 0.0, 0.0), UP, VIEW))   # 39.8 degrees off an axis with a 28 degree outer cone


def test_zero_direction_takes_down():
    world = _v(0.4, 0.0, 0.2)
    a = sample(_props(2, position_ws=(0.0, 3.0, 0.0), direction_ws=(0.0, 0.0, 0.0)), world, UP, VIEW)
    b = sample(_props(2, position_ws=(0.0, 3.0, 0.0), direction_ws=(0.0, -1.0, 0.0)), world, UP, VIEW)
    assert a[0].min() > 0
    _same(a, b)
    # the rect's forward too (safe_forward): facing down, lit from above
    r0 = sample(_props(3, position_ws=(0.0, 2.0, 0.0), direction_ws=(0.0, 0.0, 0.0), up_ws=(0.0, 0.0, 1.0)), world, UP, VIEW)
    r1 = sample(_props(3, position_ws=(0.0, 2.0, 0.0), direction_ws=(0.0, -1.0, 0.0), up_ws=(0.0, 0.0, 1.0)), world, UP, VIEW)
    assert r0[0].min() > 0
    _same(r0, r1)


RECT = dict(position_ws=(0.0, 2.0, 0.0), direction_ws=(0.0, -1.0, 0.0), up_ws=(0.0, 0.0, 1.0), range=8.0)
# basis_from_forward_and_hint of RECT by hand: right = cross(up_ref, fwd) = (1, 0, 0), up = cross(fwd, right) = (0, 0, 1)


def test_rect_behind_and_in_plane_is_zero():
    p = _props(3, **RECT)
    down = _v(0.0, -1.0, 0.0)
    _zero(sample(p, _v(0.3, 2.5, 0.1), down, VIEW))           # behind the emitter's plane, surface facing it
    _zero(sample(p, _v(2.0, 2.0, 0.0), _v(-1.0, 0.0, 0.0), VIEW))   # exactly in the plane: emission_facing == 0


def test_rect_off_the_edge_uses_the_clamped_corner():
    p = _props(3, color=(0.7, 0.8, 0.9), **RECT)
    world = _v(3.0, 0.5, 2.0)
    emit = _v(0.0, 2.0, 0.0)
    emit = (emit + _v(1.0, 0.0, 0.0) * F(0.8)).astype(F)      # ux clamped to +half_ext.x
    emit = (emit + _v(0.0, 0.0, 1.0) * F(0.5)).astype(F)      # uy clamped to +half_ext.y
    L, dist = _from_emit(p, emit, world)
    facing = max(_dot(_v(0.0, -1.0, 0.0), -L), F(0.0))
    gain = F(F(0.65) + F(F(0.55) * facing))
    want = _tail(p, L, dist, gain, 26.0, 0.26, UP, VIEW)
    got = sample(p, world, UP, VIEW)
    assert got[0].min() > 0
    _same(got, want)


TUBE = dict(position_ws=(0.0, 2.0, 0.0), right_ws=(1.0, 0.0, 0.0), range=6.0)


def _tube_want(p, end, world):
    L, dist = _from_emit(p, end, world)
    soft = min(max(F(F(1.0) - F(dist / max(F(p["range"]), F(0.1)))), F(0.0)), F(1.0))
    return _tail(p, L, dist, F(F(0.75) + F(F(0.35) * soft)), 22.0, 0.20, UP, VIEW)


def test_tube_past_the_end_uses_the_endpoint():
    p = _props(4, tube_half_length=1.0, **TUBE)
    world = _v(3.0, 0.0, 0.5)
    got = sample(p, world, UP, VIEW)
    assert got[0].min() > 0
    _same(got, _tube_want(p, _v(1.0, 2.0, 0.0), world))


def test_dist_equal_to_range_is_zero():
    _zero(sample(_props(1, position_ws=(0.0, 3.0, 0.0), range=3.0), _v(0.0, 0.0, 0.0), UP, VIEW))
    _zero(sample(_props(2, position_ws=(0.0, 3.0, 0.0), range=3.0), _v(0.0, 0.0, 0.0), UP, VIEW))
    _zero(sample(_props(4, tube_half_length=1.0, **{**TUBE, "range": 2.0}), _v(0.5, 0.0, 0.0), UP, VIEW))
    r = _props(3, **{**RECT, "range": 2.0})
    _zero(sample(r, _v(0.2, 0.0, 0.1), UP, VIEW))
    assert sample(_props(3, **{**RECT, "range": 2.5}), _v(0.2, 0.0, 0.1), UP, VIEW)[0].min() > 0   # (inside: lit)


def test_small_extents_take_the_clamps():
    world = _v(3.0, 0.0, 0.5)
    p = _props(4, tube_half_length=0.02, **TUBE)                       # half length floor 0.1
    _same(sample(p, world, UP, VIEW), _tube_want(p, (_v(0.0, 2.0, 0.0) + _v(1.0, 0.0, 0.0) * F(0.1)).astype(F), world))
    r = _props(3, rect_half_extents=(0.01, 0.02), **RECT)              # half extent floor 0.05
    w2 = _v(3.0, 0.5, 2.0)
    emit = ((_v(0.0, 2.0, 0.0) + _v(1.0, 0.0, 0.0) * F(0.05)).astype(F) + _v(0.0, 0.0, 1.0) * F(0.05)).astype(F)
    L, dist = _from_emit(r, emit, w2)
    gain = F(F(0.65) + F(F(0.55) * max(_dot(_v(0.0, -1.0, 0.0), -L), F(0.0))))
    got = sample(r, w2, UP, VIEW)
    assert got[0].min() > 0
    _same(got, _tail(r, L, dist, gain, 26.0, 0.26, UP, VIEW))


# ---- shs_light_pack_culling --------------------------------------------------------------------
def test_pack_points_equals_make_point_lights_bitwise():
    from shs_gpu import scene_lib
    from shs_gpu.lib_path import make_point_lights, make_point_props, pack_culling
    rng = np.random.default_rng(5)
    n = 300
    args = (rng.uniform(-30, 30, (n, 3)), rng.uniform(0.0, 9.0, n), rng.uniform(-0.2, 1.0, (n, 3)), rng.uniform(-0.5, 2.0, n))
    for kw in ({}, dict(attenuation_model=2, power=2.5, bias=0.5, cutoff=0.1), dict(attenuation_model=0, power=0.0, bias=0.0)):
        assert pack_culling(make_point_props(*args, **kw)).tobytes() == make_point_lights(*args, **kw).tobytes()
    c4 = scene_lib.c4_lights(64)
    typed = scene_lib.c4_lights_typed(64)
    typed["type"] = 1
    assert pack_culling(typed).tobytes() == c4.tobytes()


def _record(**kw):
    from shs_gpu.lib_path import LIGHT_DTYPE
    r = np.zeros(1, LIGHT_DTYPE)
    for k, val in kw.items():
        r[k] = val
    return r


def test_pack_spot_rect_tube_hand_computed_records():
    from shs_gpu.lib_path import light_props, pack_culling
    hp = F(np.pi / 2)
    # Spot: make_spot_culling_light (light_types.hpp:351-379) after SpotLightModel::pack_for_culling's clamps
    p = light_props(1, 2)
    p["position_ws"], p["range"], p["direction_ws"] = (1.0, 2.0, 3.0), 5.0, (0.0, 0.0, 2.0)
    p["inner_angle_rad"], p["outer_angle_rad"], p["color"], p["intensity"] = 0.3, 0.5, (0.5, -1.0, 2.0), 1.5
    inner = min(max(min(max(F(0.3), F(0.02)), F(hp - F(0.02))), F(0.01)), F(hp - F(0.01)))
    outer = F(0.5)
    want = _record(position_range=(1, 2, 3, 5), color_intensity=(0.5, 0.0, 2.0, 1.5),
                   direction_spot=(0, 0, 1, _libm.cosf(inner)), axis_spot_outer=(1, 0, 0, _libm.cosf(outer)),
                   up_shape_x=(0, 1, 0, 0), shape_attenuation=(0, 1.0, 0.05, 0.0), type_shape_flags=(2, 2, 7, 1),
                   cull_sphere=(1, 2, 3, 5), cull_aabb_min=(-4, -3, -2, 1), cull_aabb_max=(6, 7, 8, 1))
    assert pack_culling(p).tobytes() == want.tobytes()
    # Rect: rect_area_light_culling_obb (:267-290): dir (0,-1,0), right (1,0,0), up (0,0,1); centre = position +
    # dir * range/2; half extents (hx + range, hy + range, range/2); the record's direction is -dir
    p = light_props(1, 3)
    p["position_ws"], p["range"], p["direction_ws"], p["up_ws"] = (1.0, 2.0, 3.0), 4.0, (0.0, -1.0, 0.0), (0.0, 0.0, 1.0)
    hx, hy = F(F(0.8) + F(4.0)), F(F(0.5) + F(4.0))
    rad = np.sqrt(F(F(F(hx * hx) + F(hy * hy)) + F(4.0)))
    want = _record(position_range=(1, 2, 3, 4), color_intensity=(1, 1, 1, 1), direction_spot=(-0.0, 1.0, -0.0, 1.0),
                   # glm::cross((0,0,1), (0,-1,0)).z = 0 * -1 - 0 * 0 = -0, kept by every later step
                   axis_spot_outer=(1, 0, -0.0, 0), up_shape_x=(0, 0, 1, hx), shape_attenuation=(hy, 1.0, 0.05, 0.0),
                   type_shape_flags=(3, 3, 7, 1), cull_sphere=(1, 0, 3, rad),
                   cull_aabb_min=(F(1) - hx, -2, F(3) - hy, 1), cull_aabb_max=(F(1) + hx, 2, F(3) + hy, 1))
    got = pack_culling(p)
    for k in want.dtype.names:
        assert got[k].tobytes() == want[k].tobytes(), (k, got[k], want[k])
    # Tube: tube_area_light_culling_capsule (:301-315): a, b = position -/+ axis * 1.5, radius = max(range, radius)
    p = light_props(1, 4)
    p["position_ws"], p["range"], p["right_ws"], p["tube_half_length"] = (1.0, 2.0, 3.0), 3.0, (0.0, 2.0, 0.0), 1.5
    want = _record(position_range=(1, 2, 3, 3), color_intensity=(1, 1, 1, 1), direction_spot=(0, 1, 0, 1),
                   axis_spot_outer=(0, 1, 0, 0), up_shape_x=(0, 1, 0, 1.5), shape_attenuation=(3.0, 1.0, 0.05, 0.0),
                   type_shape_flags=(4, 4, 7, 1), cull_sphere=(1, 2, 3, 4.5), cull_aabb_min=(-2, -2.5, 0, 1),
                   cull_aabb_max=(4, 6.5, 6, 1))
    got = pack_culling(p)
    for k in want.dtype.names:
        assert got[k].tobytes() == want[k].tobytes(), (k, got[k], want[k])


def test_pack_rejects_other_types():
    from shs_gpu.lib_path import light_props, pack_culling
    for t in (0, 5):
        with pytest.raises(ValueError):
            pack_culling(light_props(2, t))


# ---- ABI surface ------------------------------------------------------------------------------
def test_abi_surface():
    import shs_gpu
    from shs_gpu import _abi, lib_path
    L = shs_gpu.lib()
    for name in ("shs_light_pack_culling", "shs_lights_upload_typed", "shs_group_lights_upload_typed"):
        assert getattr(L, name).restype is ctypes.c_int
    assert L.shs_abi_version() == 1
    assert ref_lib().ref_sizeof(0) == ctypes.sizeof(_abi.LightPropsC) == lib_path.LIGHT_PROPS_DTYPE.itemsize == 128
    assert ref_lib().ref_sizeof(1) == ctypes.sizeof(_abi.CullingLightC) == lib_path.LIGHT_DTYPE.itemsize == 160
    assert len(lib_path.LIGHT_PROPS_DTYPE.names) == len(_abi.LightPropsC._fields_)
    for name, (cname, _ct) in zip(lib_path.LIGHT_PROPS_DTYPE.names, _abi.LightPropsC._fields_):
        assert name == cname
        assert lib_path.LIGHT_PROPS_DTYPE.fields[name][1] == getattr(_abi.LightPropsC, cname).offset
    assert _abi.PROGRAM_FORWARD_PLUS_TYPED == lib_path.PROGRAM_FORWARD_PLUS_TYPED == 6
    header = open(os.path.join(os.path.dirname(HERE), "include", "shs_gpu.h")).read()
    assert "#define SHS_PROGRAM_FORWARD_PLUS_TYPED 6" in header
