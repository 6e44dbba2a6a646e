"""Stale-tile clears (SHS_OPT_LEGACY_STALE_CLEAR): a legacy batch clears only the raster tiles an earlier
batch of the context left non-clear, and falls back to clearing every idle tile whenever the library
cannot vouch for what the planes hold.

One context (option on, the default) runs through sequences of batches; every frame of every batch is
compared bit for bit -- colour, depth, and the present / prequant planes where enabled -- with the same
batch on a context that clears fully every time (option 0).  Sizes: 322x181 (W % 4 != 0, partial tiles
on both edges), 320x184 (the 16-B strip path), 33x17 and 1x1."""
import ctypes

import numpy as np
import pytest

from helpers import FLT_MAX
from test_batch import _owned_mask, _poses
from test_gpu_parity import _hair_soup, _identity_draw

pytestmark = pytest.mark.gpu

SIZES = [(322, 181), (320, 184), (33, 17), (1, 1)]


@pytest.fixture(scope="module")
def ref_ctx():
    """Clears every idle tile in every batch, as every batch did before the option existed."""
    import shs_gpu
    ctx = shs_gpu.Context(0)
    ctx.set_stale_clear(False)
    yield ctx
    ctx.close()


@pytest.fixture()
def ctx():
    import shs_gpu
    c = shs_gpu.Context(0)
    yield c
    c.close()


def _frame(W, H, **kw):
    import shs_gpu
    return shs_gpu.Frame(W, H, **kw)


def _sets(n, W, H, shading=3):
    """Pose sets A and B of n frames each: B continues A's sweep, so the object has moved."""
    _, fd = _poses(2 * n, shading=shading, width=W, height=H)
    return fd[:n], fd[n:]


def _planes(c, frame, k):
    """Every enabled plane of frame k as uint32 / float bit patterns, with the pixels of other shards
    zeroed (a shard writes only its own tiles)."""
    col, z = c.resolve_frame(k)
    out = {"color": np.ascontiguousarray(col).view(np.uint32).reshape(frame.height, frame.width),
           "depth": z.view(np.uint32)}
    if frame.present:
        out["present"] = np.ascontiguousarray(c.resolve_present(k)).view(np.uint32).reshape(frame.height, frame.width)
    if frame.prequant:
        out["prequant"] = c.resolve_prequant(k).view(np.uint32)
    if frame.shard_count > 1:
        m = _owned_mask(frame)
        canvas = {"color": m[::-1], "depth": m, "present": m, "prequant": m[::-1][..., None]}
        out = {name: np.where(canvas[name], a, 0) for name, a in out.items()}
    return out


def _check(c, ref, frame, fds, label=""):
    """Render the batch on both contexts; every frame, every enabled plane, bit-exact."""
    c.render_batch(frame, fds)
    ref.render_batch(frame, fds)
    for k in range(len(fds)):
        got, want = _planes(c, frame, k), _planes(ref, frame, k)
        for name in want:
            assert np.array_equal(got[name], want[name]), f"{label}: frame {k}: {name} differs from a full-clear render"


def _assert_all_clear(c, frame, n):
    rgba = np.frombuffer(bytes(frame.clear_color), np.uint32)[0]
    for k in range(n):
        p = _planes(c, frame, k)
        assert (p["color"] == rgba).all() and (p["present"] == rgba).all(), f"frame {k}: colour not clear"
        assert (p["depth"] == np.float32(FLT_MAX).view(np.uint32)).all(), f"frame {k}: depth not clear"
        assert (p["prequant"] == 0).all(), f"frame {k}: prequant not clear"


def _hair_sets(W, H, n_frames, n_tris, seed):
    from shs_gpu.scene import Mesh
    out = []
    for s in range(2 * n_frames):
        pos, nrm = _hair_soup(np.random.default_rng(seed + s), W, H, n_tris)
        out.append([_identity_draw(Mesh(pos, nrm), 3)])
    return out[:n_frames], out[n_frames:]


@pytest.mark.parametrize("mode", [1, 2], ids=["scan", "bins"])
@pytest.mark.parametrize("W,H", SIZES)
def test_moved_object_then_empty_batch(ctx, ref_ctx, W, H, mode):
    """A -> B (the object moved: A's tiles go stale) -> a batch without draws (every plane entirely
    clear) -> A, with all four planes enabled."""
    n = 3
    A, B = _sets(n, W, H)
    frame = _frame(W, H, present=True, prequant=True)
    for c in (ctx, ref_ctx):
        c.set_raster_mode(mode)
    try:
        _check(ctx, ref_ctx, frame, A, "A")
        _check(ctx, ref_ctx, frame, B, "B")
        _check(ctx, ref_ctx, frame, [[] for _ in range(n)], "empty")
        _assert_all_clear(ctx, frame, n)
        _check(ctx, ref_ctx, frame, A, "A again")
    finally:
        ref_ctx.set_raster_mode(0)


@pytest.mark.parametrize("mode", [1, 2], ids=["scan", "bins"])
@pytest.mark.parametrize("W,H", SIZES[:2])
def test_hair_slivers_ghost_fragments_outside_their_boxes(ctx, ref_ctx, W, H, mode):
    """Sliver soups: ghost fragments make tiles busy outside every bbox; they go stale like any other."""
    n = 2
    A, B = _hair_sets(W, H, n, 1500, 500)
    frame = _frame(W, H, present=True, prequant=True)
    for c in (ctx, ref_ctx):
        c.set_raster_mode(mode)
    try:
        _check(ctx, ref_ctx, frame, A, "A")
        assert ctx.stats()["ghost_fragments"] > 0
        _check(ctx, ref_ctx, frame, B, "B")
        _check(ctx, ref_ctx, frame, [[] for _ in range(n)], "empty")
        _assert_all_clear(ctx, frame, n)
        _check(ctx, ref_ctx, frame, A, "A again")
    finally:
        ref_ctx.set_raster_mode(0)


@pytest.mark.parametrize("W,H", SIZES[:2])
def test_clear_colour_change(ctx, ref_ctx, W, H):
    A, _ = _sets(3, W, H)
    _check(ctx, ref_ctx, _frame(W, H), A, "black")
    _check(ctx, ref_ctx, _frame(W, H, clear_color=(10, 200, 30, 255)), A, "green")
    _check(ctx, ref_ctx, _frame(W, H, clear_color=(10, 200, 30, 255)), A, "green again")
    _check(ctx, ref_ctx, _frame(W, H), A, "black again")


@pytest.mark.parametrize("plane", ["present", "prequant"])
def test_plane_off_on_off_on(ctx, ref_ctx, plane):
    """A plane that a batch does not write keeps older contents: enabling it again clears it fully."""
    W, H = 322, 181
    A, B = _sets(3, W, H)
    for i, (on, fds) in enumerate([(False, A), (True, B), (False, A), (True, A), (True, B)]):
        _check(ctx, ref_ctx, _frame(W, H, **{plane: on}), fds, f"step {i} {plane}={on}")


def test_frame_count_sequence(ctx, ref_ctx):
    W, H = 322, 181
    _, fd = _poses(10, width=W, height=H)
    for i, (lo, n) in enumerate([(0, 3), (3, 5), (1, 2), (5, 5), (0, 5)]):
        _check(ctx, ref_ctx, _frame(W, H), fd[lo:lo + n], f"step {i}: {n} frames")


def test_shard_sequence(ctx, ref_ctx):
    W, H = 322, 181
    A, B = _sets(3, W, H)
    for i, (rank, count, fds) in enumerate([(0, 1, A), (1, 3, B), (1, 3, A), (0, 1, A), (0, 1, B)]):
        _check(ctx, ref_ctx, _frame(W, H, shard_rank=rank, shard_count=count), fds, f"step {i}: shard {rank}/{count}")


def test_size_sequence(ctx, ref_ctx):
    for i, (W, H) in enumerate([(322, 181), (33, 17), (322, 181), (320, 184), (322, 181)]):
        A, B = _sets(3, W, H)
        _check(ctx, ref_ctx, _frame(W, H), A, f"step {i}: {W}x{H} A")
        _check(ctx, ref_ctx, _frame(W, H), B, f"step {i}: {W}x{H} B")


@pytest.mark.parametrize("mode", [1, 2], ids=["scan", "bins"])
def test_overflowing_batch_between_ordinary_ones(ctx, ref_ctx, mode):
    """A batch that overflows the spill and fragment lists is re-issued; the re-issue starts from the
    map the overflowed pass left (a superset of the non-clear tiles)."""
    W, H = 322, 181
    A, B = _sets(2, W, H)
    hair, _ = _hair_sets(W, H, 2, 3000, 700)
    frame = _frame(W, H)
    for c in (ctx, ref_ctx):
        c.set_raster_mode(mode)
    try:
        _check(ctx, ref_ctx, frame, A, "A")
        ctx.set_bin_capacity(1)
        ctx.set_overflow_capacities(spill=8, frags=8)
        _check(ctx, ref_ctx, frame, hair, "overflowing")
        assert ctx.stats()["ghost_fragments"] > 8
        _check(ctx, ref_ctx, frame, B, "B")
        _check(ctx, ref_ctx, frame, A, "A again")
    finally:
        ref_ctx.set_raster_mode(0)


def test_pipelined_batches_between_ordinary_ones(ctx, ref_ctx):
    """SHS_OPT_LEGACY_PIPELINE batches (more than 6 draws in all, scan mode) always clear fully, and so
    does the batch after them."""
    W, H = 322, 181
    A, B = _sets(8, W, H)
    frame = _frame(W, H)
    _check(ctx, ref_ctx, frame, A, "A")
    _check(ctx, ref_ctx, frame, B, "B")
    ctx.set_legacy_pipeline(True)
    _check(ctx, ref_ctx, frame, A, "pipelined A")
    ctx.render_batch(frame, B)          # its raster is still pending when the next batch is enqueued
    _check(ctx, ref_ctx, frame, A, "pipelined A after pending B")
    ctx.set_legacy_pipeline(False)
    _check(ctx, ref_ctx, frame, B, "B after the pipeline")
    _check(ctx, ref_ctx, frame, A, "A again")


def _hip():
    import torch  # noqa: F401  (maps torch's HIP runtime, the one libshs_gpu binds)
    hip = ctypes.CDLL("libamdhip64.so.7")
    hip.hipMemset.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t]
    return hip


@pytest.mark.parametrize("W,H", SIZES[:2])
def test_external_write_through_handed_out_pointers(ctx, ref_ctx, W, H):
    """The planes are overwritten through the pointers shs_device_framebuffers / shs_present_device hand
    out; the same batch rendered again is right (the hand-out makes the next batch clear fully)."""
    n = 3
    A, _ = _sets(n, W, H)
    frame = _frame(W, H, present=True)
    hip = _hip()
    _check(ctx, ref_ctx, frame, A, "A")
    _check(ctx, ref_ctx, frame, A, "A again")
    color, depth = ctx.device_framebuffers()
    present = ctx.present_device(0)
    for ptr in (color, depth, present):
        assert hip.hipMemset(ctypes.c_void_p(ptr), 0xA5, n * W * H * 4) == 0
    assert hip.hipDeviceSynchronize() == 0
    _check(ctx, ref_ctx, frame, A, "A after the external write")
    # one pointer alone
    present = ctx.present_device(1)
    assert hip.hipMemset(ctypes.c_void_p(present), 0x3C, W * H * 4) == 0
    assert hip.hipDeviceSynchronize() == 0
    _check(ctx, ref_ctx, frame, A, "A after a write into frame 1's staging")


def test_packed_tiles_unpacked_into_the_legacy_target(ctx, ref_ctx):
    import torch
    W, H = 322, 181
    A, _ = _sets(3, W, H)
    frame = _frame(W, H, present=True)
    _check(ctx, ref_ctx, frame, A, "A")
    for target in (ctx.TARGET_LEGACY, ctx.TARGET_PRESENT):
        words = ctx.tiles_rank_words(target, 0, 1)
        buf = torch.full((words,), 0x5A5A5A5A, dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()
        ctx.tiles_unpack(target, 0, 1, buf.data_ptr())
        ctx.synchronize()
        plane = "present" if target == ctx.TARGET_PRESENT else "color"
        assert (_planes(ctx, frame, 0)[plane] == 0x5A5A5A5A).all()   # the unpack did overwrite frame 0
        _check(ctx, ref_ctx, frame, A, f"A after an unpack into target {target}")
        del buf


def test_the_path_is_live(ctx, ref_ctx):
    """Cleared-tile counts: the second of two identical batches clears nothing, a moved object clears
    some tiles, an invalidation brings the full count back; option 0 clears the full count always."""
    W, H = 322, 181
    n = 3
    A, B = _sets(n, W, H)
    frame = _frame(W, H)
    n_rt = ((W + 31) // 32) * ((H + 7) // 8)
    ctx.render_batch(frame, A)
    first = ctx.cleared_tiles()
    assert 0 < first < n * n_rt
    ctx.render_batch(frame, A)
    assert ctx.cleared_tiles() == 0
    ctx.render_batch(frame, B)
    assert 0 < ctx.cleared_tiles() < first
    ctx.render_batch(frame, A)
    assert 0 < ctx.cleared_tiles() < first
    ctx.device_framebuffers()            # an invalidation
    ctx.render_batch(frame, A)
    assert ctx.cleared_tiles() == first
    ctx.render_batch(frame, A)
    assert ctx.cleared_tiles() == 0
    ctx.set_stale_clear(False)
    for _ in range(2):
        ctx.render_batch(frame, A)
        assert ctx.cleared_tiles() == first
    ctx.set_stale_clear(True)
    ctx.render_batch(frame, A)
    assert ctx.cleared_tiles() == 0      # full clears keep the map: the planes are still vouched for
    for _ in range(3):
        ref_ctx.render_batch(frame, A)
        assert ref_ctx.cleared_tiles() == first
