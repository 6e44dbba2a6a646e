"""Inputs shared by tests/test_lib_reference.py (oracle == compiled reference, CPU) and
tests/test_lib_reference_gpu.py (kernel vs compiled reference): the uniform sweep as a fixed parameter
table, and the synthetic PassTonemap / PassMotionBlur inputs.

The sweep scene is the C5 scene (floor + Suzanne) at 96x64 with a rendered shadow map of at most 64^2.
Every row overrides ShaderUniforms fields of both draws; `gpu=True` marks the rows of the GPU set, which
are the rows whose REFERENCE HDR stays below GPU_HDR_CAP (asserted by both test files)."""
import numpy as np

SWEEP_W, SWEEP_H = 96, 64
# The GPU set compares HDR at the suite's absolute 1e-5 (helpers.assert_float_close).  That is met by
# a float32 result only below 8.0: the top of the binade of the brightest channel the suite already
# passes at 1e-5 (Blinn-Phong C5, 5.54), where one ulp is 4.8e-7.  A condition on the reference alone.
GPU_HDR_CAP = 8.0

_DEFAULTS = dict(program=0, metallic=None, roughness=None, ao=None, base=None, lcol=(1.0, 1.0, 1.0), inten=1.0,
                 ldir="sun", bias=(0.0008, 0.0015), pcf_r=2, pcf_step=1.0, strength=1.0, sm=(64, 64), lvp="true",
                 tex=None, gpu=False)


def _row(name, **kw):
    assert not set(kw) - set(_DEFAULTS), kw
    return dict(_DEFAULTS, name=name, **kw)


def _explicit_rows():
    rows = []
    for p, tag in ((0, "pbr"), (1, "bp")):
        # material: below, at and above the clamps
        for m in (-0.5, 0.0, 1.0, 1.7):
            rows.append(_row(f"{tag}-metallic{m}", program=p, metallic=m, gpu=True))
        for r in (-0.2, 0.0, 0.02, 0.04, 1.0, 1.6):
            rows.append(_row(f"{tag}-rough{r}", program=p, roughness=r, gpu=True))
        for a in (-0.3, 0.0, 1.0, 2.5):
            rows.append(_row(f"{tag}-ao{a}", program=p, ao=a, gpu=(a != 1.0)))
        rows.append(_row(f"{tag}-base-neg", program=p, base=(-0.4, 0.5, 1.8), gpu=True))
        rows.append(_row(f"{tag}-base-big", program=p, base=(2.5, -1.0, 0.3), metallic=0.6, gpu=True))
        # light
        rows.append(_row(f"{tag}-lcol-neg", program=p, lcol=(1.0, -0.5, 0.7), gpu=True))
        for i in (0.0, 1.0, 5.0):
            rows.append(_row(f"{tag}-inten{i}", program=p, inten=i, gpu=(i == 0.0)))
        rows.append(_row(f"{tag}-inten5-smooth", program=p, inten=5.0, roughness=0.02, metallic=1.0))
        rows.append(_row(f"{tag}-ldir-zero", program=p, ldir="zero", gpu=True))
        rows.append(_row(f"{tag}-ldir-zero-noshadow", program=p, ldir="zero", sm=None, gpu=True))
    # shadow: bias, PCF radius x step, strength, map shapes, receivers outside / on the border
    for i, b in enumerate([(0.0, 0.0), (0.0008, 0.0015), (0.05, 0.05), (0.0, 0.05), (0.05, 0.0)]):
        rows.append(_row(f"bias{b[0]}-{b[1]}", program=i % 2, bias=b, gpu=(i in (0, 2))))
    for i, r in enumerate((-1, 0, 1, 2, 3)):
        for j, s in enumerate((0.4, 1.0, 1.5, 2.5, 3.0)):
            rows.append(_row(f"pcf{r}-step{s}", program=(i + j) % 2, pcf_r=r, pcf_step=s,
                             gpu=(r in (-1, 3) and s in (1.5, 2.5)) or (r == 1 and s == 0.4)))
    for i, s in enumerate((-0.5, 0.0, 0.3, 1.0, 1.5)):
        rows.append(_row(f"strength{s}", program=i % 2, strength=s, gpu=(s in (-0.5, 0.3, 1.5))))
    rows.append(_row("sm-48x20", sm=(48, 20), pcf_r=1, gpu=True))
    rows.append(_row("sm-20x48-bp", program=1, sm=(20, 48), pcf_step=2.0))
    # a 1x1 map holds its clear value 1.0 (every caster is degenerate in it): a negative constant bias
    # moves z_test across it, so part of the receivers is shadowed
    rows.append(_row("sm-1x1", sm=(1, 1), bias=(-0.52, 0.0), pcf_r=0, gpu=True))
    rows.append(_row("sm-1x1-pcf2-bp", program=1, sm=(1, 1), bias=(-0.52, 0.0015), pcf_r=2, pcf_step=2.5, gpu=True))
    rows.append(_row("sm-2x1", sm=(2, 1), bias=(-0.52, 0.0), pcf_r=1))
    rows.append(_row("lvp-outside", lvp="outside", pcf_r=1, gpu=True))
    rows.append(_row("lvp-outside-bp", program=1, lvp="outside", pcf_r=0))
    # the border column of the map holds the clear value too (the light camera has a margin): negative bias again
    rows.append(_row("lvp-border", lvp="border", bias=(-0.52, 0.0), pcf_r=2, pcf_step=1.5, gpu=True))
    rows.append(_row("lvp-border-bp", program=1, lvp="border", bias=(-0.52, 0.0015), pcf_r=0))
    rows.append(_row("sm-synthetic-7x5", sm="synthetic", pcf_r=2, pcf_step=2.5))
    rows.append(_row("sm-synthetic-7x5-bp", program=1, sm="synthetic", pcf_r=1))
    # textures with uvs outside [0,1) and negative (the C5 floor's run from -2.25 to 4.25)
    for i, t in enumerate(((1, 1), (1, 7), (6, 1), (5, 4))):
        rows.append(_row(f"tex{t[0]}x{t[1]}", program=i % 2, tex=t, gpu=(t in ((1, 1), (1, 7)))))
        rows.append(_row(f"tex{t[0]}x{t[1]}-b", program=(i + 1) % 2, tex=t, base=(1.4, 0.9, -0.2), gpu=(t == (1, 7))))
    return rows


def _seeded_rows(n=24, seed=0x5EED5):
    """Mixed rows from a fixed seed: the table is the same in every run."""
    rng = np.random.default_rng(seed)
    rows = []
    for i in range(n):
        sm = [(64, 64), (33, 64), (64, 64), (5, 3), (1, 1)][int(rng.integers(0, 5))]
        rows.append(_row(
            f"mix{i}", program=int(rng.integers(0, 2)), metallic=float(rng.uniform(-0.5, 1.5)),
            roughness=float(rng.uniform(-0.2, 1.4)), ao=float(rng.uniform(-0.5, 2.0)),
            base=tuple(float(v) for v in rng.uniform(-0.5, 2.0, 3)), lcol=tuple(float(v) for v in rng.uniform(-0.5, 1.5, 3)),
            inten=float(rng.choice([0.0, 1.0, 1.0, 5.0, 5.0])), ldir="zero" if i % 8 == 7 else "sun",
            bias=(float(rng.choice([0.0, 0.0008, 0.05, -0.52])), float(rng.choice([0.0, 0.0015, 0.05]))),
            pcf_r=int(rng.integers(-1, 4)), pcf_step=float(rng.uniform(0.4, 3.0)), strength=float(rng.uniform(-0.5, 1.5)),
            sm=sm, lvp=["true", "true", "outside", "border"][int(rng.integers(0, 4))],
            tex=[None, (1, 1), (1, 7), (6, 1), (5, 4)][int(rng.integers(0, 5))]))
    return rows


SWEEP = _explicit_rows() + _seeded_rows()
SWEEP_GPU = [r for r in SWEEP if r["gpu"]]
assert len({r["name"] for r in SWEEP}) == len(SWEEP)


def synthetic_shadow_map():
    """A 7x5 map of seeded depths around the receivers' light-space depth (CPU-only rows)."""
    return np.random.default_rng(77).uniform(0.35, 0.75, size=(5, 7)).astype(np.float32)


def light_viewproj_of(row, lvp):
    """The draws' light_viewproj for a row, from the shadow pass's own (bytes pass through every side)."""
    from shs_gpu.lib_path import mat_mul
    lvp = np.asarray(lvp, np.float32)
    if row["lvp"] == "true":
        return lvp
    m = np.eye(4, dtype=np.float32)
    if row["lvp"] == "outside":      # ndc x scaled by 3 and shifted: most receivers leave [0,1] in u (lit)
        m[0, 0], m[0, 3] = 3.0, 0.75
    else:                            # "border": clip x = clip w, so u = 1.0 exactly: the last texel column
        m[0, :] = (0.0, 0.0, 0.0, 1.0)
    return mat_mul(np.ascontiguousarray(m.T).reshape(16), lvp)   # column-major storage


def sweep_scene(row):
    """-> (frame, draws, shadow) for a row; shadow = None or (size, sun, casters) for the shadow pass whose
    light camera `wire(row, draws, lvp)` then installs."""
    from shs_gpu import scene_lib
    tex = row["tex"]
    frame, draws, casters, sun, _ = scene_lib.c5_scene(SWEEP_W, SWEEP_H, program=row["program"], textured=tex is not None,
                                                       floor_tex=tex or (1, 1), monkey_tex=tex or (1, 1))
    for d in draws:
        for key, field in (("metallic", "metallic"), ("roughness", "roughness"), ("ao", "ao"), ("base", "base_color")):
            if row[key] is not None:
                setattr(d, field, row[key])
        d.light_color, d.light_intensity = row["lcol"], row["inten"]
        if row["ldir"] == "zero":
            d.light_dir_ws = (0.0, 0.0, 0.0)
        d.shadow_bias_const, d.shadow_bias_slope = row["bias"]
        d.shadow_pcf_radius, d.shadow_pcf_step, d.shadow_strength = row["pcf_r"], row["pcf_step"], row["strength"]
    if row["sm"] is None:
        return frame, draws, None
    size = (64, 64) if row["sm"] == "synthetic" else row["sm"]
    return frame, draws, (size, sun, casters)


def wire(row, draws, lvp):
    from shs_gpu import scene_lib
    scene_lib.wire_shadow(draws, light_viewproj_of(row, lvp))


# ---- PassTonemap / PassMotionBlur inputs -------------------------------------------------------------
TONEMAP_GAMMAS = [2.2, 1.0, 1.8, 0.5, 0.0, -1.0]    # test_post.py::test_thresholds_match_reference_bytes


def synthetic_hdr(W=256, H=64):
    """The HDR target of test_post.py::test_tonemap_synthetic_hdr_exact: values within +-6 ulps of every
    byte boundary (gamma 2.2), NaN / +-inf / negative / denormal / huge, the rest seeded noise."""
    import shs_gpu
    thr = shs_gpu.Context.tonemap_thresholds(2.2)
    vals = []
    for t in thr[1:]:
        if np.isfinite(t) and 0 < t < 1:
            s0 = np.float32(t / (1.0 - t))
            vals += list(s0 + np.arange(-6, 7, dtype=np.float32) * np.spacing(s0))
    vals += [np.nan, np.inf, -np.inf, -0.0, 0.0, 1e-45, 1e-38, 3e38, -5.0, 1e6]
    rng = np.random.default_rng(3)
    flat = np.array(vals, np.float32)
    hdr = rng.uniform(-0.5, 8.0, size=(H, W, 4)).astype(np.float32)
    n = min(flat.size, H * W * 3)
    rgb = hdr[..., :3].reshape(-1).copy()
    rgb[:n] = flat[:n]
    hdr[..., :3] = rgb.reshape(H, W, 3)
    hdr[..., 3] = 1.0
    assert np.isnan(hdr).any() and np.isinf(hdr).any()
    return hdr


def nonfinite_motion(W=160, H=96):
    """The motion plane of test_post.py::test_motion_blur_nonfinite_motion_exact."""
    rng = np.random.default_rng(11)
    mot = rng.uniform(-40, 40, size=(H, W, 2)).astype(np.float32)
    special = np.array([np.nan, np.inf, -np.inf, 3e38, -3e38, 1e20, np.nan, 0.0], np.float32)
    sel = rng.integers(0, special.size, size=(H, W, 2))
    mask = rng.random((H, W, 2)) < 0.3
    mot[mask] = special[sel[mask]]
    return mot


def about_shadow(row):
    """Rows that are about the shadow term: their frames must show some, but not all, receivers shadowed."""
    return row["name"].startswith(("bias", "pcf", "strength", "sm-", "lvp-"))
