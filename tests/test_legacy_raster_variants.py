"""The legacy raster's kernel variants against each other and the CPU oracle.

raster_tile and raster_group (csrc/shs_legacy.hip) are built from one set of helpers -- staging, the pair
layouts and the pair loop, the winner fetch, shading and the pixel store -- that every k_raster
instantiation and k_pipe run.  Seven contexts select the variants: the per-pixel loop in scan and
bin mode, the bin-mode span pairs, the scan-mode box pairs with a work item per tile (the reference), the
tile groups with box passes and with row spans (the default), and the pipelined launch.

Every scene is a batch of two frames (a single frame keeps a work item per tile) with the present and
prequant planes on.  Each variant's planes -- colour, depth bits, present, prequant -- are compared bit for
bit with the reference variant's, and the reference variant with the oracle.
- 240 clutter triangles inside one 64x16 group at 64x16, 65x17 and 96x24: more than one staging chunk of
  64, so the winners are fetched by index, with exact z ties; four draws per frame, one per shading model.
- A 1,500-triangle soup at 96x24: more than one gather round of 1,024.
- Hair slivers at 322x181: ghost fragments.
The clutter and soup batches hold eight draws, so the pipelined context does pipeline them (batches of at
most six draws are not pipelined); it renders a batch twice, the first's raster running inside the second's
launch, and the second's planes are the ones compared."""
import functools

import numpy as np
import pytest

from test_gpu_parity import _identity_draw, _ndc_soup
from test_stale_clear import _frame, _hair_sets, _planes
from test_tile_groups import _check_oracle, _clutter

pytestmark = pytest.mark.gpu

REFERENCE = "scan-pairs"
VARIANTS = {
    "scan-pixel-loop": lambda c: (c.set_raster_mode(1), c.set_raster_loop(0)),
    "bins-pixel-loop": lambda c: (c.set_raster_mode(2), c.set_raster_loop(0)),
    "bins-pairs": lambda c: c.set_raster_mode(2),
    REFERENCE: lambda c: (c.set_raster_mode(1), c.set_tile_groups(False)),
    "scan-groups-boxes": lambda c: (c.set_raster_mode(1), c.set_group_spans(False)),
    "scan-groups-spans": lambda c: c.set_raster_mode(1),
    "scan-pipeline": lambda c: (c.set_raster_mode(1), c.set_legacy_pipeline(True)),
}
SCENES = ["clutter-64x16", "clutter-65x17", "clutter-96x24", "soup-96x24", "hair-322x181"]


@functools.lru_cache(maxsize=None)
def _scene(name):
    """(W, H, the two frames' draw lists)."""
    from shs_gpu.scene import Mesh
    kind, size = name.split("-")
    W, H = (int(v) for v in size.split("x"))
    if kind == "clutter":
        draws = [_identity_draw(_clutter(W, H, 0, 0, 60, 40 + s), s, (255 - 60 * s, 80 * s, 40, 255)) for s in range(4)]
        return W, H, [draws, draws[::-1]]
    if kind == "soup":
        fds = []
        for seed in (51, 52):
            pos, nrm = _ndc_soup(np.random.default_rng(seed), W, H, 1500)
            parts = [Mesh(np.ascontiguousarray(pos[i::4]), np.ascontiguousarray(nrm[i::4])) for i in range(4)]
            fds.append([_identity_draw(m, (seed + i) % 4) for i, m in enumerate(parts)])
        return W, H, fds
    A, _ = _hair_sets(W, H, 2, 1500, 500)
    return W, H, A


@pytest.fixture(scope="module")
def contexts():
    import shs_gpu
    cs = {}
    try:
        for name, configure in VARIANTS.items():
            cs[name] = shs_gpu.Context(0)
            configure(cs[name])
        yield cs
    finally:
        for c in cs.values():
            c.close()


def _render(contexts, variant, scene):
    """Every enabled plane of both frames, and the batch's statistics."""
    W, H, fds = _scene(scene)
    frame = _frame(W, H, present=True, prequant=True)
    c = contexts[variant]
    if variant == "scan-pipeline":
        c.render_batch(frame, fds)   # its raster runs inside the next launch
    c.render_batch(frame, fds)
    return [_planes(c, frame, k) for k in range(len(fds))], c.stats()


@pytest.fixture(scope="module")
def reference(contexts):
    """The reference variant's planes and statistics per scene, rendered once."""
    cache = {}

    def get(scene):
        if scene not in cache:
            cache[scene] = _render(contexts, REFERENCE, scene)
        return cache[scene]
    return get


@pytest.mark.parametrize("variant", [v for v in VARIANTS if v != REFERENCE])
@pytest.mark.parametrize("scene", SCENES)
def test_variant_matches_reference(contexts, reference, scene, variant):
    want, _ = reference(scene)
    got, _ = _render(contexts, variant, scene)
    for k, (g, w) in enumerate(zip(got, want)):
        assert set(g) == set(w) == {"color", "depth", "present", "prequant"}
        for name in w:
            assert np.array_equal(g[name], w[name]), f"{variant}: {scene}: frame {k}: {name} differs from {REFERENCE}"


@pytest.mark.parametrize("scene", SCENES)
def test_reference_matches_oracle(contexts, reference, oracle_mod, scene):
    W, H, fds = _scene(scene)
    planes, stats = reference(scene)
    assert stats["covered_pixels"] > 0
    if scene.startswith("hair"):
        assert stats["ghost_fragments"] > 0   # the case cannot pass by having no ghosts
    _check_oracle(contexts[REFERENCE], oracle_mod, _frame(W, H), fds[0])
