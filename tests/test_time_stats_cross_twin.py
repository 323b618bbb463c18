"""The rule of the cross sums, the moment layers and the stride of the time statistics (cmc_fluid_solver_amd/time_stats.py:
FS3D_OPT_TIME_STATS_CROSS, FS3D_OPT_OUTPUT_MOMENT, FS3D_OPT_TIME_STATS_EVERY) on the CPU: the numpy twin against a per-cell loop
written straight from the rule, the properties the rule promises, and the driver's refusals of `--time-covariances` and
`--time-stats-every` (decided when the arguments are read: no GPU needed).
The kernels are held to the twin in test_gpu_time_stats_cross.py."""
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
PAIRS = ((0, 1), (0, 2), (1, 2), (0, 3), (1, 3), (2, 3))       # uv, uw, vw, uT, vT, wT: written out here, not read from the twin


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


def loop_layers(steps, cur, every, dtype):
    """The rule cell by cell in Python floats (IEEE double, one rounding per operation): {(source, moment): four arrays}, and N"""
    R = np.dtype(dtype).type
    out = {key: [np.zeros(SHAPE, dtype) for _ in range(4)] for key in ((1, 0), (2, 0), (2, 1), (2, 2), (3, 0))}
    counted = [s for s in range(1, len(steps) + 1) if (s - 1) % every == 0]
    N = len(counted)
    for idx in np.ndindex(*SHAPE):
        n, S1, S2, SX = 0, [0.0] * 4, [0.0] * 4, [0.0] * 6
        for s in counted:
            fields, types = steps[s - 1]
            if types[idx] != grids.NODE_IN:
                continue
            n += 1
            x = [float(fields[v][idx]) for v in range(4)]
            with np.errstate(all="ignore"):
                for v in range(4):
                    S1[v] = S1[v] + x[v]
                    S2[v] = S2[v] + np.float64(x[v]) * np.float64(x[v])
                for p, (a, b) in enumerate(PAIRS):
                    SX[p] = SX[p] + np.float64(x[a]) * np.float64(x[b])
        if n == 0:
            for v in range(4):
                out[1, 0][v][idx] = cur[v][idx]
            continue
        with np.errstate(all="ignore"):
            dn = np.float64(n)
            m = [np.float64(S1[v]) / dn for v in range(4)]
            var = []
            for v in range(4):
                d = np.float64(S2[v]) / dn - m[v] * m[v]
                var.append(np.float64(0.0) if d < 0.0 else d)
            cov = [np.float64(SX[p]) / dn - m[a] * m[b] for p, (a, b) in enumerate(PAIRS)]
            tke = np.float64(0.5) * ((var[0] + var[1]) + var[2])
            for v in range(4):
                out[1, 0][v][idx] = R(m[v])
                out[2, 0][v][idx] = R(var[v])
            for v in range(3):
                out[2, 1][v][idx] = R(cov[v])
                out[2, 2][v][idx] = R(cov[3 + v])
            out[2, 1][3][idx] = R(tke)
            out[2, 2][3][idx] = R(var[3])
            out[3, 0][3][idx] = R(dn / np.float64(N))
    return out, N


def bits(a):
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def same(a, b):
    return a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("every", [1, 3])
def test_twin_equals_the_per_cell_loop(every, dtype):
    steps, cur = random_case(dtype)
    assert any((a[1] != b[1]).any() for a, b in zip(steps, steps[1:])), "types change between steps"
    mags = np.abs(np.concatenate([np.ravel(f) for fields, _ in steps for f in fields]).astype(np.float64))
    assert mags.min() < 1e-18 and mags.max() > 1e18
    ts = TS.TimeStats(SHAPE, 2, cross=True, every=every)
    taken = [ts.add(fields, types) for fields, types in steps]
    want, N = loop_layers(steps, cur, every, dtype)
    assert ts.N == N == (7 if every == 1 else 3) and sum(taken) == N
    for (source, moment), fields in want.items():
        got = ts.layer(source, cur, moment)
        for v in range(4):
            assert same(got[v], fields[v]), (source, moment, v)
    # the moment is read for source 2 only
    for source in (1, 3):
        for a, b in zip(ts.layer(source, cur, 2), ts.layer(source, cur)):
            assert np.array_equal(bits(a), bits(b))
    with pytest.raises(ValueError):
        ts.layer(2, cur, 3)
    # some covariance is negative: nothing clamps it
    assert any((q[np.isfinite(q)] < 0).any() for q in ts.layer(2, cur, 1)[:3] + ts.layer(2, cur, 2)[:3])


@pytest.mark.parametrize("dtype", DTYPES)
def test_small_integer_constant_fields_have_every_covariance_exactly_zero(dtype):
    types = np.full(SHAPE, grids.NODE_IN, np.uint8)
    consts = [dtype(3), dtype(-7), dtype(12), dtype(293)]
    fields = [np.full(SHAPE, c, dtype) for c in consts]
    ts = TS.TimeStats(SHAPE, 2, cross=True)
    for _ in range(7):
        ts.add(fields, types)
    for moment in (0, 1, 2):
        for q in ts.layer(2, fields, moment):
            assert (q == 0).all(), moment


@pytest.mark.parametrize("dtype", DTYPES)
def test_covariance_is_not_clamped_and_k_is_half_the_sum_of_the_variances(dtype):
    """v = -u exactly: x_u * x_v = -(x_u * x_u) and m_u * m_v = -(m_u * m_u) bit for bit (a sign flips no rounding), so cov(u, v) is
    the negative of the unclamped S2 / n - m * m of u"""
    rng = np.random.default_rng(9)
    types = np.full(SHAPE, grids.NODE_IN, np.uint8)
    ts = TS.TimeStats(SHAPE, 2, cross=True)
    for _ in range(NSTEPS):
        u = rng.uniform(-2, 2, SHAPE).astype(dtype)
        ts.add([u, -u, rng.uniform(-2, 2, SHAPE).astype(dtype), rng.uniform(280, 300, SHAPE).astype(dtype)], types)
    cur = [np.zeros(SHAPE, dtype)] * 4
    stress, var = ts.layer(2, cur, 1), ts.layer(2, cur, 0)
    m = ts.S1[0] / np.float64(NSTEPS)
    unclamped = ts.S2[0] / np.float64(NSTEPS) - m * m
    assert np.array_equal(bits(stress[0]), bits((-unclamped).astype(dtype)))
    assert (stress[0] < 0).any(), "negative somewhere: no clamp was applied"
    # k from the double variances, rounded once
    dn = np.float64(NSTEPS)
    dv = []
    for v in range(3):
        mv = ts.S1[v] / dn
        d = ts.S2[v] / dn - mv * mv
        dv.append(np.where(d < 0.0, 0.0, d))
    assert np.array_equal(bits(stress[3]), bits((0.5 * ((dv[0] + dv[1]) + dv[2])).astype(dtype)))
    assert (stress[3] > 0).all()
    for v in range(3):
        assert np.array_equal(bits(var[v]), bits(dv[v].astype(dtype)))
    assert np.array_equal(bits(ts.layer(2, cur, 2)[3]), bits(var[3]))


@pytest.mark.parametrize("dtype", DTYPES)
def test_every_third_of_seven_steps_counts_steps_1_4_and_7(dtype):
    steps, cur = random_case(dtype, seed=6)
    ts = TS.TimeStats(SHAPE, 2, cross=True, every=3)
    taken = [ts.add(fields, types) for fields, types in steps]
    assert taken == [True, False, False, True, False, False, True] and ts.N == 3 and ts.candidates == 7
    picked = TS.TimeStats(SHAPE, 2, cross=True)
    for k in (0, 3, 6):
        picked.add(*steps[k])
    assert np.array_equal(ts.n, picked.n) and ts.n.max() <= 3
    for source, moment in ((1, 0), (2, 0), (2, 1), (2, 2), (3, 0)):
        for a, b in zip(ts.layer(source, cur, moment), picked.layer(source, cur, moment)):
            assert np.array_equal(bits(a), bits(b)), (source, moment)
    # a new window starts its count again: the first step always counts
    ts.reset()
    assert ts.N == 0 and ts.candidates == 0 and not any(s.any() for s in ts.SX)
    assert ts.add(*steps[1]) and not ts.add(*steps[2])
    for bad in (0, -1, 2 ** 20 + 1, 1.5):
        with pytest.raises(ValueError):
            TS.TimeStats(SHAPE, 2, every=bad)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mode", [1, 2])
def test_defaults_give_the_old_results_bit_for_bit(mode, dtype):
    """cross=False, every=1 against the rule as it stood: n, S1, S2 as recursive sums, and the three sources"""
    steps, cur = random_case(dtype, seed=7)
    old = TS.TimeStats(SHAPE, mode)
    new = TS.TimeStats(SHAPE, mode, cross=False, every=1)
    crossed = TS.TimeStats(SHAPE, mode, cross=True)
    for fields, types in steps:
        for ts in (old, new, crossed):
            ts.add(fields, types)
    assert old.SX is None and new.SX is None and (crossed.SX is None) == (mode == 1)
    n = np.zeros(SHAPE, np.uint32)
    S1 = [np.zeros(SHAPE) for _ in range(4)]
    S2 = [np.zeros(SHAPE) for _ in range(4)]
    with np.errstate(all="ignore"):
        for fields, types in steps:
            fluid = types == grids.NODE_IN
            n += fluid
            for v in range(4):
                x = fields[v].astype(np.float64)
                S1[v] = np.where(fluid, S1[v] + x, S1[v])
                S2[v] = np.where(fluid, S2[v] + x * x, S2[v])
    for ts in (old, new, crossed):
        assert np.array_equal(ts.n, n) and ts.N == NSTEPS
        for v in range(4):
            assert np.array_equal(ts.S1[v].view(np.uint64), S1[v].view(np.uint64))
            if mode == 2:
                assert np.array_equal(ts.S2[v].view(np.uint64), S2[v].view(np.uint64))
    for source in ((1, 2, 3) if mode == 2 else (1, 3)):
        ref = old.layer(source, cur)
        for ts in (new, crossed):
            for a, b in zip(ref, ts.layer(source, cur, 0)):
                assert np.array_equal(bits(a), bits(b))
    for ts in (old, new) + ((crossed,) if mode == 1 else ()):
        with pytest.raises(ValueError):
            ts.layer(2, cur, 1)
    assert TS.MOMENTS == {"variance": 0, "stress": 1, "heatflux": 2}


def test_cross_kernels_use_no_scratch(tmp_path):
    """The compiler's resource report for gfx950 (no GPU needed): the four MODE 3 accumulation kernels and the layer kernel keep
    their arrays in registers (a thread of the vector form holds 16 doubles), and stay within the 128 VGPRs of 4 waves per SIMD"""
    import re
    src = os.path.join(B.CSRC, "kernels_stats.hip")
    r = subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")] + B.FLAGS + ["-Rpass-analysis=kernel-resource-usage", "-c", src, "-o",
                        str(tmp_path / "kernels_stats.o")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    report = {}
    for name, vgprs, scratch in re.findall(r"Function Name: (\S+).*?VGPRs: (\d+).*?ScratchSize \[bytes/lane\]: (\d+)", r.stderr, flags=re.S):
        report[name] = (int(vgprs), int(scratch))
    cross = [n for n in report if re.search(r"k_time_stats_v[14]I[fd]Li3E", n)]
    layer = [n for n in report if "k_time_stats_layer" in n]
    assert len(cross) == 4 and len(layer) == 2, sorted(report)
    for n in cross + layer:
        assert report[n][1] == 0 and report[n][0] <= 128, (n, report[n])
    assert all(s == 0 for _, s in report.values()), report


def test_driver_refuses_the_new_words_when_it_reads_the_arguments(built, tmp_path):
    driver = B.build_driver()
    data, cfgf = (os.path.join(INPUTS, f) for f in ("box_pipe_2D_data.txt", "box_pipe_2D_config.txt"))
    prefix = str(tmp_path / "o")
    for words, text in ((["--time-covariances"], "--time-covariances: needs --time-stats variance"),
                        (["--time-stats", "mean", "--time-covariances"], "--time-covariances: needs --time-stats variance"),
                        (["--time-covariances", "--time-stats", "mean"], "--time-covariances: needs --time-stats variance"),
                        (["--time-stats", "variance", "--time-covariances", "--time-stats-every", "0"], "--time-stats-every"),
                        (["--time-stats", "variance", "--time-stats-every", "2.5"], "--time-stats-every"),
                        (["--time-stats", "variance", "--time-stats-every", "two"], "--time-stats-every"),
                        (["--time-stats", "variance", "--time-stats-every"], "--time-stats-every")):
        r = subprocess.run([driver, data, prefix, cfgf, "align", "GPU"] + words, capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and text in r.stderr, words
        assert "Grid =" not in r.stdout, "refused before the geometry is loaded"
        assert not os.path.exists(prefix + "_res.nc") and not os.path.exists(prefix + "_stats.nc")
    usage = subprocess.run([driver], capture_output=True, text=True, timeout=60).stdout
    assert "[--time-stats mean|variance] [--time-covariances] [--time-stats-every K]" in usage
