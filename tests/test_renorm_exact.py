"""The second normalise of an already normalised vector (renorm_inv, csrc/shs_device.hpp): for d = dot3(v, v)
whose bit pattern lies in a window around 1.0f the reciprocal square root is integer arithmetic on the
pattern, and must be the two correctly rounded IEEE operations' result bit for bit.

CPU part: the helper's lines, cut from shs_device.hpp between its markers and compiled for the host with the
oracle's flags, against 1.0f / sqrtf(d) for every pattern of the window and 64 either side, and the general
path outside it; and the cap that keeps the fast path running: dot3(normalize3(v)) stays inside the window.

gpu part: Context.legacy_shade_samples over normal sums searched (float32 numpy, the kernels' operation
order) so that the second normalise meets every k that occurs, plus the sums that must take the general path,
against tests/legacy_shaders_ref.  The normal visualiser's floats are the normalised normal itself: bit for
bit.  Toon's are IEEE operations and one pow decision: bit for bit away from the specular step.  The others
keep the suite's colour bar."""
import ctypes
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import helpers
from test_legacy_shaders_ref import (BLINN, CAM, COLOR, DEPTH_VIS, F, GOOCH, LIGHT, NORMAL_VIS, OREN, TOON, excusable,
                                     ref_samples, same_bits)

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(os.path.dirname(HERE), "leisure-software-renderer_amd", "csrc", "shs_device.hpp")
ONE = 0x3F800000
PHONG = 2

HOST_PRELUDE = r"""
#include <math.h>
#include <stdint.h>
#include <string.h>
#define SHS_RENORM_HOST 1
#define SHS_RENORM_FN static inline
static inline uint32_t SHS_RENORM_BITS(float x) { uint32_t u; memcpy(&u, &x, 4); return u; }
static inline float SHS_RENORM_FLOAT(uint32_t u) { float x; memcpy(&x, &u, 4); return x; }
"""
HOST_EXPORTS = r"""
extern "C" {
int32_t rn_kmin(void) { return RENORM_KMIN; }
int32_t rn_kmax(void) { return RENORM_KMAX; }
void rn_run(int64_t n, const float *d, float *inv, float *window, float *general, int32_t *in_window) {
    for (int64_t i = 0; i < n; ++i) {
        inv[i] = renorm_inv(d[i]);
        window[i] = renorm_inv_window(d[i]);
        volatile float s = sqrtf(d[i]);          /* the two IEEE operations, each rounded once */
        general[i] = 1.0f / s;
        in_window[i] = renorm_in_window(d[i]) ? 1 : 0;
    }
}
}
"""


@functools.lru_cache(maxsize=None)
def host_lib(tmp):
    text = open(HEADER).read()
    m = re.search(r"// \[renorm-begin\]\n(.*?)// \[renorm-end\]", text, re.S)
    assert m, "the helper's markers"
    src = os.path.join(tmp, "renorm_host.cpp")
    with open(src, "w") as f:
        f.write(HOST_PRELUDE + m.group(1) + HOST_EXPORTS)
    out = os.path.join(tmp, "librenorm_host.so")
    subprocess.run([os.environ.get("CXX", "g++"), "-O3", "-ffp-contract=off", "-fno-fast-math", "-std=c++17", "-fPIC", "-shared",
                    "-o", out, src, "-lm"], check=True)
    L = ctypes.CDLL(out)
    L.rn_kmin.restype = L.rn_kmax.restype = ctypes.c_int32
    L.rn_run.argtypes = [ctypes.c_int64] + [ctypes.c_void_p] * 5
    return L


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return host_lib(str(tmp_path_factory.mktemp("renorm")))


def run(L, bits):
    d = np.ascontiguousarray(np.asarray(bits, np.uint32)).view(F)
    out = [np.empty(d.size, F) for _ in range(3)] + [np.empty(d.size, np.int32)]
    L.rn_run(d.size, d.ctypes.data, *[o.ctypes.data for o in out])
    return d, out[0], out[1], out[2], out[3].astype(bool)


def window(L):
    kmin, kmax = L.rn_kmin(), L.rn_kmax()
    assert kmin <= -7 and kmax >= 3, "the window holds every k seen"
    assert kmin >= -40 and kmax <= 20, "the window lies inside the verified range"
    return kmin, kmax


def test_window_is_the_two_ieee_operations_bit_for_bit(host):
    kmin, kmax = window(host)
    k = np.arange(kmin - 64, kmax + 64 + 1, dtype=np.int64)
    d, inv, win, gen, inw = run(host, (ONE + k).astype(np.uint32))
    assert np.array_equal(inw, (k >= kmin) & (k <= kmax))
    assert inw.sum() == kmax - kmin + 1
    assert np.array_equal(inv.view(np.uint32), gen.view(np.uint32)), "renorm_inv differs from 1.0f / sqrtf(d)"
    # the integer formula alone, over the window: it is what the lanes inside it return
    assert np.array_equal(win.view(np.uint32)[inw], gen.view(np.uint32)[inw])
    # and it is a formula, not a copy of the general path: outside the verified range it goes wrong
    far = run(host, np.array([ONE + 4096, ONE - 4096], np.uint32))
    assert not np.array_equal(far[2].view(np.uint32), far[3].view(np.uint32))
    # numpy's float32 sqrt and divide agree with the host's
    with np.errstate(all="ignore"):
        assert np.array_equal((F(1.0) / np.sqrt(d)).view(np.uint32), gen.view(np.uint32))


def test_outside_the_window_takes_the_general_path(host):
    window(host)
    pats = [0x00000000, 0x80000000, 0x00000001, 0x007FFFFF, 0x80000001, 0x00800000, 0x7F800000, 0xFF800000, 0x7FC00000,
            0xFFC00000, 0x7F800001, 0xBF800000, 0xBF800001, 0xBF7FFFFF, 0xC0000000, 0x3F000000, 0x40000000, 0x3F7FFF00,
            0x3F800100, 0x7F7FFFFF, 0x2EDBE6FF, 0x501502F9]
    d, inv, _, gen, inw = run(host, np.array(pats, np.uint32))
    assert not inw.any()
    assert np.array_equal(np.isnan(inv), np.isnan(gen))
    ok = ~np.isnan(gen)
    assert np.array_equal(inv.view(np.uint32)[ok], gen.view(np.uint32)[ok])
    assert np.isinf(inv[0]) and inv[0] > 0 and np.isinf(inv[1]) and inv[1] < 0      # 1 / sqrt(+-0)
    assert np.isnan(inv[5 + 6]) and inv[6] == 0.0 and np.isnan(inv[7])             # -1, +inf, -inf


def _dot(a):
    return (a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]) + a[:, 2] * a[:, 2]


def _normalize(v):
    return v * (F(1.0) / np.sqrt(_dot(v)))[:, None]


def _k_of(ns):
    """The second normalise's k of float32 normal sums (finite, nonzero): pattern of dot3(normalize3(ns)) - ONE."""
    return _dot(_normalize(ns)).view(np.uint32).astype(np.int64) - ONE


def test_dot_of_a_normalised_vector_stays_inside_the_window(host):
    """>= 1e7 seeded vectors at scales 1e-3, 1 and 50: the cap that keeps the fast path from silently not running."""
    kmin, kmax = window(host)
    rng = np.random.default_rng(16)
    seen = set()
    n = 0
    for scale in (1e-3, 1.0, 50.0):
        for _ in range(4):
            v = (rng.standard_normal((900_000, 3)) * scale).astype(F)
            k = _k_of(v)
            n += k.size
            assert k.min() >= kmin and k.max() <= kmax, (scale, int(k.min()), int(k.max()))
            seen.update(np.unique(k).tolist())
    assert n >= 10_000_000
    assert set(range(-5, 4)) <= seen, sorted(seen)   # (-6 .. 3 here; -7 about once in 2e7: RARE_SUMS)


# ---- gpu part -------------------------------------------------------------------------------------------------
# k = -7 turns up about once in 2e7 random sums: six found by the search below run over 1.8e8, kept as bit patterns
RARE_SUMS = np.array([[0xbaa50d42, 0xbac9b2d2, 0xb902ba57], [0xbf3ce62e, 0x3dd106d3, 0xbe027ad2], [0xc1c71ff8, 0xc1b50f22, 0x3f90d3e1],
                      [0xbfa44acf, 0xbfcb6d8a, 0xbeebc20a], [0xc2887ea2, 0x414084c9, 0x415b4cc5], [0xb917082e, 0x3ab7aebb, 0xb999621b]],
                     np.uint32).view(F)


@functools.lru_cache(maxsize=None)
def searched_sums():
    """Normal sums whose second normalise meets every k that occurs (at least -7 .. 3), up to 360 of each where
    the search finds them, at three scales; then the sums of the general path."""
    rng = np.random.default_rng(1600)
    per = {}
    for scale in (1e-3, 1.0, 50.0):
        v = (rng.standard_normal((1_500_000, 3)) * scale).astype(F)
        k = _k_of(v)
        for kk in np.unique(k).tolist():
            got = per.setdefault(kk, [])
            if len(got) < 3:
                got.append(v[k == kk][:120])
    assert (_k_of(RARE_SUMS) == -7).all()
    per[-7] = per.get(-7, []) + [RARE_SUMS]
    assert set(range(-7, 4)) <= set(per), sorted(per)
    ns = np.vstack([a for kk in sorted(per) for a in per[kk]])
    den = np.float32(1e-40)
    general = np.array([[0, 0, 0], [np.nan, 0.3, 0.5], [0.2, np.nan, np.nan], [1e30, 1e30, 1e30], [1e30, 0, 0], [1e-30, 1e-30, 1e-30],
                        [0, 1e-30, 0], [den, den, den], [den, 0, -den], [1e30, 1e-30, den], [np.inf, 1, 1], [-1e-30, 2e-30, 1e-30],
                        [1e-20, -3e-20, 2e-20], [-2e19, 1e19, 1e18]], F)
    return ns, general


def _phong_numpy(light_dir, cam, color, ns, wp):
    """phong_shading.cpp's FS in float32 numpy (shade_interp's comments name the lines)."""
    d3 = lambda a, b: (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]
    nz = lambda v: v * (F(1.0) / np.sqrt(d3(v, v)))[..., None]
    gmax = lambda x, y: np.where(x < y, y, x)
    with np.errstate(all="ignore"):
        norm = nz(nz(ns))
        L = nz(-np.asarray(light_dir, F))
        V = nz(np.asarray(cam, F) - wp)
        diff = gmax(d3(norm, L), F(0.0))
        I = -L
        refl = I - (norm * d3(norm, I)[:, None]) * F(2.0)
        spec = np.power(gmax(d3(V, refl), F(0.0)).astype(np.float64), 32.0).astype(F)
        s = (F(0.15) + diff * F(1.0)) + (F(0.8) * spec) * F(1.0)
        oc = np.asarray(color[:3], F) / F(255.0)
        res = s[:, None] * oc
        return (np.where(res < 0, F(0.0), np.where(res > 1, F(1.0), res)) * F(255.0)).astype(F)


@pytest.fixture(scope="module")
def ctx():
    import shs_gpu
    c = shs_gpu.Context(0)
    yield c
    c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("model", [PHONG, BLINN, TOON, GOOCH, OREN, NORMAL_VIS, DEPTH_VIS])
def test_samples_over_every_k_and_the_general_path(ctx, model):
    found, general = searched_sums()
    ns = np.vstack([found, general])
    n = ns.shape[0]
    assert 2000 <= n <= 8000
    rng = np.random.default_rng(77)
    wp = rng.uniform(-6.0, 6.0, size=(n, 3)).astype(F)
    cz = rng.uniform(-5.0, 60.0, size=n).astype(F)
    light = np.asarray(LIGHT, F)
    rgba, pq = ctx.legacy_shade_samples(model, light, CAM, COLOR, ns, wp, cz)
    assert (rgba[:, 3] == 255).all() and (pq[:, 3] == 1.0).all()
    if model == PHONG:   # (not one of the reference's models: its float32 restatement)
        want = _phong_numpy(light, CAM, COLOR, ns, wp)
        assert np.array_equal(np.isnan(pq[:, :3]), np.isnan(want))
        ok = ~np.isnan(want)
        d = np.abs(pq[:, :3][ok].astype(np.float64) - want[ok])
        print(f"model {model}: max float difference {d.max():.3g} over {n} samples")
        assert d.max() <= helpers.TOL * 255.0
        return
    ref = ref_samples(model, light, CAM, COLOR, ns, wp, cz)
    assert np.array_equal(rgba[:, 3], ref["rgba"][:, 3])
    assert np.array_equal(np.isnan(pq), np.isnan(ref["prequant"]))
    keep = ~excusable(model, ref)
    assert keep.sum() >= (0.4 if model == OREN else 0.98) * n
    if model in (NORMAL_VIS, DEPTH_VIS, TOON):
        # IEEE operations alone (Toon: beside the pow decision, which the excused samples hold): the same floats
        eq = same_bits(pq, ref["prequant"])
        print(f"model {model}: {int((~eq[keep]).sum())} floats differ over {int(keep.sum())} samples")
        assert eq[keep].all()
        assert np.array_equal(rgba[keep], ref["rgba"][keep])
        if model == NORMAL_VIS:   # the general path's sums: NaN where the reference's normalise gives NaN
            g = slice(found.shape[0], n)
            assert np.isnan(pq[g][0, :3]).all() and np.isnan(pq[g][1, :3]).all()
            assert np.isfinite(pq[g][12, :3]).all()   # a denormal first dot: the second is far from 1
        return
    d = np.abs(pq[keep, :3].astype(np.float64) - ref["prequant"][keep, :3])
    d = d[~np.isnan(d)]
    print(f"model {model}: max float difference {d.max():.3g} over {int(keep.sum())} samples")
    assert d.max() <= helpers.TOL * 255.0
    d8 = np.abs(rgba[keep].astype(np.int16) - ref["rgba"][keep].astype(np.int16))
    assert d8.max(initial=0) <= 1
