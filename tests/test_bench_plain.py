"""A plain `bench.py --gpus 1 --steps N --warmup W` runs only the headline loop; every other leg is behind
--full.  --dump-outputs writes what the last timed step computed.  (CPU: which legs main() calls, with the
GPU loop replaced; GPU: one small run whose dump is compared with the same batch rendered here.)"""
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

LEGS = ("collect_pmc", "strong_legs_guarded", "seam1_pcie", "cpu_baseline")


def _main_with_fake_loop(monkeypatch, capsys, argv):
    """bench.main() with run_gpu replaced by a 0.5 s / --steps result -> (line, legs called, run_gpu's args)."""
    called, seen = [], []
    mesh = types.SimpleNamespace(n_tris=967)
    frame = types.SimpleNamespace(width=1920, height=1080)

    def fake_run_gpu(args, rank, local_rank, world, dist):
        seen.append(args)
        return (frame, [[[types.SimpleNamespace(mesh=mesh)]]], {"covered_pixels": 1000}, 0.5, args.steps,
                {"setup": 0.01, "raster": 0.2}, None, {"ms": 60.0, "batches": 8})
    results = {"collect_pmc": (None, "not run"), "strong_legs_guarded": {"strong_c4": {}}, "seam1_pcie": {"frames": 1},
               "cpu_baseline": {"value": 1.0}}
    for leg in LEGS:
        monkeypatch.setattr(bench, leg, lambda *a, _leg=leg, **k: (called.append(_leg), results[_leg])[1])
    monkeypatch.setattr(bench, "run_gpu", fake_run_gpu)
    monkeypatch.setattr(sys, "argv", ["bench.py"] + argv)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "SHS_BENCH_REHEARSE"):
        monkeypatch.delenv(k, raising=False)
    bench.main()
    line = json.loads([l for l in capsys.readouterr().out.splitlines() if l.startswith("{")][-1])
    return line, called, seen[0]


def test_plain_run_is_the_headline_loop_only(monkeypatch, capsys):
    line, called, args = _main_with_fake_loop(monkeypatch, capsys, ["--gpus", "1", "--steps", "50", "--warmup", "5"])
    assert called == []
    assert not args.full and args.dump_outputs is None and args.steps == 50 and args.warmup == 5
    assert line["steps"] == 50 and line["warmup"] == 5
    assert line["ms_per_step"] == 10.0                      # 0.5 s over the 50 timed steps
    assert line["metric"] == bench.METRIC and line["unit"] == "Mtri/s" and line["higher_is_better"] is True
    assert line["dtype"] == "f32"
    F = bench.LEGACY_FRAMES["c2"]
    assert abs(line["value"] - 967 * F * 50 / 0.5 / 1e6) < 1e-3
    for k in ("cpu_baseline", "seam1_pcie", "single_frame", "strong_c4"):
        assert k not in line


def test_full_run_adds_every_leg(monkeypatch, capsys):
    line, called, args = _main_with_fake_loop(monkeypatch, capsys, ["--full", "--steps", "50", "--warmup", "5"])
    assert called == list(LEGS)
    assert args.full
    assert line["ms_per_step"] == 10.0
    for k in ("cpu_baseline", "seam1_pcie", "strong_c4"):
        assert k in line


def test_full_legs_keep_their_own_switches(monkeypatch, capsys):
    _, called, _ = _main_with_fake_loop(monkeypatch, capsys, ["--full", "--no-pmc", "--no-cpu", "--no-pcie", "--strong", ""])
    assert called == []


def test_sample_pixels_fixed_and_in_range():
    a, b = bench.sample_pixels(1920 * 1080, 8192), bench.sample_pixels(1920 * 1080, 8192)
    assert np.array_equal(a, b) and a.size == 8192 and np.all(np.diff(a) > 0)
    assert a[0] >= 0 and a[-1] < 1920 * 1080
    assert bench.sample_pixels(100, 8192).size == 100


@pytest.mark.gpu
def test_dump_outputs_is_the_last_timed_batch(tmp_path):
    """One small C1 run (4 frames per step, 3 timed steps): the dump holds float32 / float64 arrays under
    64 MB, and they are the framebuffers of the last timed step's batch (pose set (3 - 1) % POSE_SETS)."""
    import shs_gpu
    out = tmp_path / "dump"
    F, steps = 4, 3
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--config", "c1", "--steps", str(steps),
                        "--warmup", "1", "--frames-per-step", str(F), "--ramp-ms", "0", "--dump-outputs", str(out)],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert line["steps"] == steps and line["ms_per_step"] > 0
    got = {f[:-4]: np.load(out / f) for f in sorted(os.listdir(out))}
    assert set(got) == {"sample_pixels", "color", "depth", "color_frame0", "depth_frame0"}
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert sum(a.nbytes for a in got.values()) <= 64_000_000
    frame, sets = bench.batch_poses("c1", F)
    idx = got["sample_pixels"].astype(np.int64)
    assert np.array_equal(idx, bench.sample_pixels(frame.width * frame.height, idx.size))
    with shs_gpu.Context(0) as ctx:
        ctx.render_batch(frame, sets[(steps - 1) % bench.POSE_SETS])
        for i in range(F):
            c, d = ctx.resolve_frame(i)
            assert np.array_equal(got["color"][i], c.reshape(-1, 4)[idx].astype(np.float32))
            assert np.array_equal(got["depth"][i].view(np.uint32), d.reshape(-1)[idx].view(np.uint32))
            if i == 0:
                assert np.array_equal(got["color_frame0"], c.astype(np.float32))
                assert np.array_equal(got["depth_frame0"].view(np.uint32), d.view(np.uint32))
    assert (got["depth_frame0"] < np.finfo(np.float32).max).any()      # the frame is not empty
