"""The rule of the time statistics (cmc_fluid_solver_amd/time_stats.py: FS3D_OPT_TIME_STATS, FS3D_OPT_OUTPUT_SOURCE) on the CPU: the
numpy twin against a per-cell loop written straight from the rule, the rounding bound of its mean, the properties the rule promises,
and the driver's refusal of a bad `--time-stats` word (decided when the arguments are read: no GPU needed).
The kernels are held to the twin in test_gpu_time_stats.py."""
import math
import os
import subprocess

import numpy as np
import pytest

from cmc_fluid_solver_amd import build as B
from cmc_fluid_solver_amd import grids
from cmc_fluid_solver_amd import time_stats as TS

HERE = os.path.dirname(os.path.abspath(__file__))
INPUTS = os.path.join(HERE, "golden", "inputs")
SHAPE = (5, 4, 3)
NSTEPS = 7
DTYPES = [np.float32, np.float64]


def wide_fields(rng, shape, dtype):
    """Four fields of both signs whose magnitudes span 1e-20 .. 1e20"""
    return [(rng.choice([-1.0, 1.0], shape) * 10.0 ** rng.uniform(-20, 20, shape)).astype(dtype) for _ in range(4)]


def random_case(dtype, seed=5):
    """NSTEPS steps of fields and of node types that change between the steps; cell (0, 0, 0) is never fluid, (0, 0, 1) always"""
    rng = np.random.default_rng(seed)
    steps = []
    for _ in range(NSTEPS):
        types = rng.integers(0, 4, SHAPE).astype(np.uint8)
        types[0, 0, 0] = grids.NODE_BOUND
        types[0, 0, 1] = grids.NODE_IN
        steps.append((wide_fields(rng, SHAPE, dtype), types))
    return steps, wide_fields(rng, SHAPE, dtype)


def loop_layers(steps, cur, mode, dtype):
    """The rule cell by cell in Python floats (IEEE double, one rounding per operation): {source: four arrays}"""
    R = np.dtype(dtype).type
    out = {s: [np.zeros(SHAPE, dtype) for _ in range(4)] for s in ((1, 3) if mode == 1 else (1, 2, 3))}
    N = len(steps)
    for idx in np.ndindex(*SHAPE):
        n, S1, S2 = 0, [0.0] * 4, [0.0] * 4
        for fields, types in steps:
            if types[idx] != grids.NODE_IN:
                continue
            n += 1
            for v in range(4):
                x = float(fields[v][idx])
                S1[v] = S1[v] + x
                S2[v] = S2[v] + x * x
        for v in range(4):
            if n == 0:
                out[1][v][idx] = cur[v][idx]
                continue
            m = S1[v] / float(n)
            with np.errstate(over="ignore"):
                out[1][v][idx] = R(m)
                if mode == 2:
                    var = S2[v] / float(n) - m * m
                    out[2][v][idx] = R(0.0 if var < 0.0 else var)
            if v == 3:
                out[3][v][idx] = R(float(n) / float(N))
    return out


def bits(a):
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mode", [1, 2])
def test_twin_equals_the_per_cell_loop_bit_for_bit(mode, dtype):
    steps, cur = random_case(dtype)
    assert any((a[1] != b[1]).any() for a, b in zip(steps, steps[1:])), "types change between steps"
    mags = np.abs(np.concatenate([np.ravel(f) for fields, _ in steps for f in fields]).astype(np.float64))
    assert mags.min() < 1e-18 and mags.max() > 1e18
    ts = TS.TimeStats(SHAPE, mode)
    for fields, types in steps:
        ts.add(fields, types)
    assert ts.N == NSTEPS
    want = loop_layers(steps, cur, mode, dtype)
    assert sorted(want) == ([1, 2, 3] if mode == 2 else [1, 3])
    for source, fields in want.items():
        got = ts.layer(source, cur)
        for v in range(4):
            assert got[v].dtype == np.dtype(dtype)
            assert np.array_equal(bits(got[v]), bits(fields[v])), (source, v)
    if mode == 1:
        with pytest.raises(ValueError):
            ts.layer(2, cur)


@pytest.mark.parametrize("dtype", DTYPES)
def test_mean_lies_within_the_documented_bound_of_fsum(dtype):
    steps, cur = random_case(dtype, seed=6)
    ts = TS.TimeStats(SHAPE, 1)
    for fields, types in steps:
        ts.add(fields, types)
    got = ts.layer(1, cur)
    checked = 0
    for idx in np.ndindex(*SHAPE):
        xs = [[float(fields[v][idx]) for fields, types in steps if types[idx] == grids.NODE_IN] for v in range(4)]
        n = len(xs[0])
        if n == 0:
            continue
        for v in range(4):
            exact = math.fsum(xs[v]) / n                       # one rounding of the exact sum, one of the division: within 2 u of the true mean
            bound = TS.mean_bound(math.fsum(abs(x) for x in xs[v]), n, dtype) + 2 * 2.0 ** -53 * abs(exact)
            assert abs(float(got[v][idx]) - exact) <= bound, (idx, v)
            checked += 1
    assert checked > 100
    # the bound is a rounding bound, not a loose one: a few ulps of R for a handful of terms
    assert TS.mean_bound(7.0, 7, dtype) < 1.01 * np.finfo(dtype).eps / 2 + 8 * 2.0 ** -53


@pytest.mark.parametrize("dtype", DTYPES)
def test_constant_field_has_variance_exactly_zero(dtype):
    types = np.full(SHAPE, grids.NODE_IN, np.uint8)
    consts = [dtype(1.1), dtype(-3.3e7), dtype(1e-12), dtype(293.15)]
    if dtype == np.float64:                                     # squares that are exact in double: few significant bits
        consts = [dtype(1.5), dtype(-32500000.0), dtype(2.0 ** -40), dtype(293.25)]
    fields = [np.full(SHAPE, c, dtype) for c in consts]
    ts = TS.TimeStats(SHAPE, 2)
    for _ in range(8):                                          # n = 8: n * x and n * x^2 are exact
        ts.add(fields, types)
    var = ts.layer(2, fields)
    mean = ts.layer(1, fields)
    for v in range(4):
        assert (var[v] == 0).all() and not np.signbit(var[v]).any()
        assert (mean[v] == consts[v]).all()
    frac = ts.layer(3, fields)
    assert (frac[3] == 1).all() and all((frac[v] == 0).all() for v in range(3))


@pytest.mark.parametrize("dtype", DTYPES)
def test_cells_never_fluid_follow_the_rule_and_reset_opens_a_new_window(dtype):
    steps, cur = random_case(dtype, seed=7)
    ts = TS.TimeStats(SHAPE, 2)
    with pytest.raises(ValueError):
        ts.layer(1, cur)                                        # N = 0
    for fields, types in steps:
        ts.add(fields, types)
    never = ts.n == 0
    assert never[0, 0, 0] and not never[0, 0, 1] and ts.n[0, 0, 1] == NSTEPS
    mean, var, frac = (ts.layer(s, cur) for s in (1, 2, 3))
    for v in range(4):
        assert np.array_equal(bits(mean[v][never]), bits(cur[v][never]))
        assert (var[v][never] == 0).all() and (frac[v][never] == 0).all()
    assert np.array_equal(frac[3], (ts.n.astype(np.float64) / NSTEPS).astype(dtype))
    assert frac[3][0, 0, 1] == 1
    ts.reset()
    assert ts.N == 0 and not ts.n.any() and not any(s.any() for s in ts.S1 + ts.S2)
    for fields, types in steps[4:]:
        ts.add(fields, types)
    fresh = TS.TimeStats(SHAPE, 2)
    for fields, types in steps[4:]:
        fresh.add(fields, types)
    for s in (1, 2, 3):
        for a, b in zip(ts.layer(s, cur), fresh.layer(s, cur)):
            assert np.array_equal(bits(a), bits(b))
    with pytest.raises(ValueError):
        TS.TimeStats(SHAPE, 3)
    with pytest.raises(ValueError):
        ts.layer(4, cur)


def test_driver_refuses_a_bad_time_stats_word_when_it_reads_the_arguments(built, tmp_path):
    driver = B.build_driver()
    data, cfgf = (os.path.join(INPUTS, f) for f in ("box_pipe_2D_data.txt", "box_pipe_2D_config.txt"))
    prefix = str(tmp_path / "o")
    for words in (["--time-stats", "median"], ["--time-stats"]):
        r = subprocess.run([driver, data, prefix, cfgf, "align", "GPU"] + words, capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and "--time-stats: mean or variance" in r.stderr, words
        assert "Grid =" not in r.stdout, "refused before the geometry is loaded"
        assert not os.path.exists(prefix + "_res.nc") and not os.path.exists(prefix + "_stats.nc")
    assert "[--time-stats mean|variance]" in subprocess.run([driver], capture_output=True, text=True, timeout=60).stdout
