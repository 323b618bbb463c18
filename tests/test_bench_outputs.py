"""bench.py --dump-outputs and --full: the dump holds the current layer after the last timed step (all cells of a small grid, a
fixed seeded sample of a large one, the same sample assembled from x-slabs), a plain run prints the headline only, --full adds the
secondary figures."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_dump_indices_are_fixed_and_bounded():
    b = _bench()
    assert np.array_equal(b.dump_indices(1000), np.arange(1000))                     # a small grid: every cell
    a, c = b.dump_indices(256 ** 3), b.dump_indices(256 ** 3)
    assert a.size == b.DUMP_SAMPLE and np.array_equal(a, c)                          # same sample in every run
    assert np.all(np.diff(a) > 0) and a[0] >= 0 and a[-1] < 256 ** 3                 # sorted, distinct, in range
    assert 4 * b.DUMP_SAMPLE * 8 <= 64 << 20                                         # 4 fp64 fields fit the 64 MB bound


@pytest.mark.parametrize("world", [1, 3, 8])
def test_slab_samples_assemble_the_global_sample(world):
    from cmc_fluid_solver_amd.slab import slab_range
    b = _bench()
    nx, ny, nz = 150, 90, 80                                                         # > DUMP_SAMPLE cells: a sampled dump
    rng = np.random.default_rng(3)
    full = [rng.standard_normal((nx, ny, nz)).astype(np.float32) for _ in range(4)]
    idx = b.dump_indices(nx * ny * nz)
    assert idx.size == b.DUMP_SAMPLE
    parts = []
    for r in range(world):
        x0, x1 = slab_range(nx, r, world)
        parts.append(b.slab_sample([f[x0:x1] for f in full], x0, ny * nz, idx))
    got = [np.concatenate([p[j] for p in parts]) for j in range(4)]
    for g, f in zip(got, full):
        assert g.dtype == np.float32 and np.array_equal(g, f.ravel()[idx])


def test_steps_must_be_positive(monkeypatch):
    b = _bench()
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "0"])
    with pytest.raises(SystemExit) as e:
        b.main()
    assert e.value.code == 2


def _run(args, tmp_path):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, cwd=str(tmp_path), capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_dumps_the_last_timed_step(built, tmp_path):
    """A plain run: headline fields only; the dump equals the same step sequence driven directly through the C ABI."""
    from cmc_fluid_solver_amd import capi, grids
    b = _bench()
    n, warmup, steps = 48, 2, 12
    out = _run(["--gpus", "1", "--size", str(n), "--steps", str(steps), "--warmup", str(warmup), "--dump-outputs", "d"], tmp_path)
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in out, k
    assert out["steps"] == steps and out["ms_per_step"] > 0 and out["higher_is_better"] is True and out["dtype"] == "f32"
    assert "roofline" not in out and "cpu_baseline" not in out and "parity_check" not in out
    dumped = [np.load(str(tmp_path / "d" / (f + ".npy"))) for f in b.DUMP_FIELDS]

    g = grids.box(n, h=1.0 / (n - 1))
    s = capi.Solver(g, capi.fluid_params(np.float32, b.RE, b.PR, b.LAMBDA), np.float32, device=0)
    s.set_option(capi.OPT_SWEEP_KERNEL, 0)
    for i in list(range(warmup)) + list(range(steps)):
        s.UpdateBoundaries()
        s.TimeStep(0.1, b.NUM_GLOBAL, b.NUM_LOCAL, i % 10 == 0)
    want = s.download_layer(capi.LAYER_CUR)
    s.close()
    for d, w in zip(dumped, want):
        assert d.dtype == np.float32 and d.shape == (n ** 3,)
        assert np.array_equal(d, w.ravel())


@pytest.mark.gpu
def test_full_run_adds_the_secondary_figures(built, tmp_path):
    out = _run(["--gpus", "1", "--size", "40", "--steps", "3", "--warmup", "1", "--full"], tmp_path)
    assert out["steps"] == 3 and out["ms_per_step"] > 0
    assert "final_div_error" in out["config"]
    assert out["roofline"]["avg_launch_ms"] > 0 and out["roofline"]["device_copy_GBps"] > 0
    assert out["cpu_baseline"]["value"] > 0
    assert out["parity_check"]["exact_kernels_bit_identical"] is True
