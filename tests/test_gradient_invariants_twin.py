"""The numpy twins of the velocity-gradient invariants: layer_output.invariants (FS3D_OPT_OUTPUT_GRADIENT 1, `vector` 2 of the record
rule) and TimeStats(gradients=True) (FS3D_OPT_TIME_STATS_GRAD, FS3D_OPT_OUTPUT_GRADIENT 2), against analytic fields, against a
per-cell loop written straight from the rule, and the driver's refusals of `--time-gradients` (decided when the arguments are read:
no GPU needed).  The kernels are held to the twins in test_gpu_output_gradient.py and test_gpu_time_stats_gradients.py."""
import os
import subprocess

import numpy as np
import pytest

from cmc_fluid_solver_amd import build as B
from cmc_fluid_solver_amd import grids
from cmc_fluid_solver_amd import layer_output as LO
from cmc_fluid_solver_amd import time_stats as TS

HERE = os.path.dirname(os.path.abspath(__file__))
INPUTS = os.path.join(HERE, "golden", "inputs")
DTYPES = [np.float32, np.float64]
POW2 = (0.25, 0.125, 0.5)
GRIDS = [(13, 11, 10), (23, 13, 11), (9, 7, 70), (6, 5, 130)]       # the four grids of test_gpu_output_filter.py


def make_nodes(dims, spacing):
    """test_gpu_output_filter.make_nodes: a box with an obstacle and a corner block of NODE_OUT cells"""
    n = grids.box_with_obstacle(*dims)
    n.dx, n.dy, n.dz = spacing
    n.type[:3, :3, :3] = grids.NODE_OUT
    return n


def integer_fields(shape, dtype, seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(-63, 64, shape).astype(dtype) for _ in range(4)]


def loop_invariants(types, fields, spacing):
    """The rule, cell by cell, in scalar arithmetic of the fields' type"""
    R = fields[0].dtype.type
    two = [R(2) * R(d) for d in spacing]
    h = R(0.5)
    out = [np.zeros(types.shape, fields[0].dtype) for _ in range(3)]
    nx, ny, nz = types.shape
    for i in range(nx):
        for j in range(ny):
            for k in range(nz):
                if types[i, j, k] == grids.NODE_OUT:
                    for o in out:
                        o[i, j, k] = R(99999)
                    continue
                if types[i, j, k] != grids.NODE_IN or not (0 < i < nx - 1 and 0 < j < ny - 1 and 0 < k < nz - 1):
                    continue
                nb = [(i - 1, j, k), (i + 1, j, k), (i, j - 1, k), (i, j + 1, k), (i, j, k - 1), (i, j, k + 1)]
                if any(types[c] == grids.NODE_OUT for c in nb):
                    continue
                g = [[(fields[a][nb[2 * b + 1]] - fields[a][nb[2 * b]]) / two[b] for b in range(3)] for a in range(3)]
                div = (g[0][0] + g[1][1]) + g[2][2]
                sxy, sxz, syz = h * (g[0][1] + g[1][0]), h * (g[0][2] + g[2][0]), h * (g[1][2] + g[2][1])
                oxy, oxz, oyz = h * (g[0][1] - g[1][0]), h * (g[0][2] - g[2][0]), h * (g[1][2] - g[2][1])
                SS = ((g[0][0] * g[0][0] + g[1][1] * g[1][1]) + g[2][2] * g[2][2]) + R(2) * ((sxy * sxy + sxz * sxz) + syz * syz)
                OO = R(2) * ((oxy * oxy + oxz * oxz) + oyz * oyz)
                for o, v in zip(out, (div, h * (OO - SS), SS)):
                    assert type(v) is R
                    o[i, j, k] = v
    return out


@pytest.mark.parametrize("dtype", DTYPES)
def test_analytic_fields_give_the_stated_invariants(dtype):
    spacing = (0.5, 0.25, 0.125)
    x, y, z = np.meshgrid(*[np.arange(3) * d for d in spacing], indexing="ij")
    zero = np.zeros_like(x)
    types = np.full((3, 3, 3), grids.NODE_BOUND, np.uint8)
    types[1, 1, 1] = grids.NODE_IN
    for name, vel, want in (("rotation", (-3 * y, 3 * x, zero), (0, 9, 0)), ("shear", (3 * y, zero, zero), (0, 0, 4.5)),
                            ("plane stretch", (3 * x, -3 * y, zero), (0, -9, 18)), ("dilatation", (3 * x, 3 * y, 3 * z), (9, -13.5, 27))):
        q = LO.invariants(types, [f.astype(dtype) for f in vel], spacing)
        assert all(a.dtype == np.dtype(dtype) for a in q)
        assert tuple(float(a[1, 1, 1]) for a in q) == want, name
        for a in q:
            a[1, 1, 1] = 0
            assert not a.any(), "every other cell of the 3^3 grid is a wall: 0"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("dims", [(13, 11, 10), (6, 5, 20)])
def test_twin_equals_the_per_cell_loop_and_the_mask_is_curl_defined(dims, dtype):
    spacing = (0.3, 0.07, 0.11)
    nodes = make_nodes(dims, spacing)
    types = np.asarray(nodes.type)
    rng = np.random.default_rng(3)
    fields = [(rng.standard_normal(dims) * 10.0 ** rng.uniform(-3, 3, dims)).astype(dtype) for _ in range(4)]
    q = LO.cell_quantities(types, fields, LO.INVARIANTS, spacing)
    st = LO.stamp(types, fields)
    want = loop_invariants(types, st, spacing)
    for a, b in zip(q[:3], want):
        assert a.dtype == b.dtype and np.array_equal(a, b)
    assert np.array_equal(q[3], st[3]), "the fourth quantity stays T"
    ok = LO.curl_defined(types)
    out_cells = types == grids.NODE_OUT
    fluid = types == grids.NODE_IN
    assert ok.any() and (fluid & ~ok).any() and out_cells.any()
    for a in q[:3]:
        assert (a[out_cells] == 99999).all() and (a[~ok & ~out_cells] == 0).all()
    assert (q[2][ok] > 0).all(), "S:S of a random field on the cells that carry it"
    with pytest.raises(ValueError):
        LO.cell_quantities(types, fields, LO.INVARIANTS)           # no spacing
    with pytest.raises(ValueError):
        LO.cell_quantities(types, fields, 3, spacing)


@pytest.mark.parametrize("dims", GRIDS)
def test_integer_fields_are_exact_in_fp32(dims):
    nodes = make_nodes(dims, POW2)
    f64 = integer_fields(dims, np.float64, 21)
    f32 = [f.astype(np.float32) for f in f64]
    q32 = LO.cell_quantities(nodes.type, f32, LO.INVARIANTS, POW2)
    q64 = LO.cell_quantities(nodes.type, f64, LO.INVARIANTS, POW2)
    ok = LO.curl_defined(nodes.type)
    biggest = 0.0
    for a, b in zip(q32, q64):
        assert a.dtype == np.float32 and np.array_equal(a.astype(np.float64), b)
        biggest = max(biggest, float(np.abs(b[ok]).max()))
    assert 1e3 < biggest <= 4.5e5
    # box sums of such values are exact in double whatever the order: the box mean of fp32 equals that of fp64
    for outdims in ((5, 4, 7), (1, 1, 1)):
        V32, T32 = LO.layer_output(nodes.type, f32, outdims, LO.BOX, LO.INVARIANTS, POW2)
        V64, T64 = LO.layer_output(nodes.type, f64, outdims, LO.BOX, LO.INVARIANTS, POW2, exact_sum=True)
        assert np.array_equal(V32, V64.astype(np.float32)) and np.array_equal(T32, T64)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cuts", [[(0, 12), (12, 23)], [(0, 11), (11, 12), (12, 23)], [(0, 1), (1, 9), (9, 16), (16, 23)]])
def test_slab_partials_and_finish_equal_the_global_record(cuts, dtype):
    dims = (23, 13, 11)
    nodes = make_nodes(dims, POW2)
    fields = integer_fields(dims, dtype, 22)
    assert any(x1 - x0 == 1 for x0, x1 in cuts) or len(cuts) == 2
    for filter in (LO.POINT, LO.BOX):
        for outdims in ((0, 0, 0), (5, 4, 7), (4, 3, 3), (50, 3, 4)):
            per_rank = [LO.slab_partials(nodes.type, fields, cuts, r, outdims, filter, LO.INVARIANTS, POW2) for r in range(len(cuts))]
            V, T = LO.finish_slabs(nodes.type, fields, cuts, per_rank, outdims, LO.INVARIANTS, POW2)
            eV, eT = LO.layer_output(nodes.type, fields, outdims, filter, LO.INVARIANTS, POW2)
            assert np.array_equal(V, eV) and np.array_equal(T, eT), (filter, outdims)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("every", [1, 2])
def test_time_stats_gradients_equal_a_direct_evaluation_per_step(every, dtype):
    dims = (9, 8, 10)
    spacing = (0.3, 0.07, 0.11)
    A, Bn = grids.box_with_obstacle(*dims, lo=0.25, hi=0.6), grids.box_with_obstacle(*dims, lo=0.4, hi=0.75)
    tA, tB = np.asarray(A.type), np.asarray(Bn.type)
    assert (LO.curl_defined(tA) != LO.curl_defined(tB)).any()
    rng = np.random.default_rng(5)
    steps = [([rng.uniform(-2, 2, dims).astype(dtype) for _ in range(4)], tB if k in (2, 3) else tA) for k in range(5)]
    ts = TS.TimeStats(dims, 1, every=every, gradients=True, spacing=spacing)
    ng = np.zeros(dims, np.uint32)
    G = [np.zeros(dims, np.float64) for _ in range(3)]
    for k, (fields, types) in enumerate(steps):
        assert ts.add(fields, types) == (k % every == 0)
        if k % every:
            continue
        ok = LO.curl_defined(types)
        inv = loop_invariants(types, fields, spacing)
        ng += ok.astype(np.uint32)
        for v in range(3):
            G[v] = np.where(ok, G[v] + inv[v].astype(np.float64), G[v])
    assert np.array_equal(ts.ng, ng) and all(np.array_equal(a, b) for a, b in zip(ts.G, G))
    assert 0 < ng.max() == ts.N and (ng[ng > 0].min() < ts.N), "cells defined on some steps only"
    cur = steps[-1][0]
    Q = ts.gradient_layer(cur)
    for v in range(3):
        want = np.zeros(dims, dtype)
        seen = ng > 0
        want[seen] = (G[v][seen] / ng[seen].astype(np.float64)).astype(dtype)
        assert Q[v].dtype == np.dtype(dtype) and np.array_equal(Q[v], want)
    assert np.array_equal(Q[3], ts.layer(TS.MEAN, cur)[3])
    # a new window
    ts.reset()
    assert ts.N == 0 and not ts.ng.any() and not any(g.any() for g in ts.G)


def test_refusals_of_the_twin():
    dims = (5, 5, 5)
    with pytest.raises(ValueError):
        TS.TimeStats(dims, 1, gradients=True)                      # no spacing
    plain = TS.TimeStats(dims, 1)
    assert plain.ng is None and plain.G is None
    types = np.asarray(grids.box(*dims).type)
    fields = [np.ones(dims, np.float32)] * 4
    plain.add(fields, types)
    with pytest.raises(ValueError):
        plain.gradient_layer(fields)                               # the window holds no gradient sums
    ts = TS.TimeStats(dims, 1, gradients=True, spacing=POW2)
    with pytest.raises(ValueError):
        ts.gradient_layer(fields)                                  # no step yet
    with pytest.raises(ValueError):
        LO.layer_output(types, fields, vector=LO.INVARIANTS)       # no spacing
    with pytest.raises(ValueError):
        LO.layer_output(types, fields, vector=3, spacing=POW2)


def test_driver_refuses_time_gradients_when_it_reads_the_arguments(built, tmp_path):
    driver = B.build_driver()
    data, cfgf = (os.path.join(INPUTS, f) for f in ("box_pipe_2D_data.txt", "box_pipe_2D_config.txt"))
    prefix = str(tmp_path / "o")
    for words, text in ((["GPU", "--time-gradients"], "--time-gradients: needs --time-stats"),
                        (["GPU", "--time-gradients", "--output-filter", "box"], "--time-gradients: needs --time-stats"),
                        (["GPU", "2", "--time-stats", "mean", "--time-gradients"], "--time-gradients: single GPU only"),
                        (["--time-stats", "variance", "--time-gradients", "GPU", "2"], "--time-gradients: single GPU only")):
        r = subprocess.run([driver, data, prefix, cfgf, "align"] + words, capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and text in r.stderr, words
        assert "Grid =" not in r.stdout, "refused before the geometry is loaded"
        assert not os.path.exists(prefix + "_res.nc") and not os.path.exists(prefix + "_stats.nc")
    usage = subprocess.run([driver], capture_output=True, text=True, timeout=60).stdout
    assert "[--time-stats-every K] [--time-gradients]" in usage
