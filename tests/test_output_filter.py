"""The rule of the filtered and derived result records (cmc_fluid_solver_amd/layer_output.py: FS3D_OPT_OUTPUT_FILTER,
FS3D_OPT_OUTPUT_VECTOR) on the CPU: the numpy twin against a loop written straight from the rule, the properties the rule
promises, and the driver's refusal of `--output-filter box` on x-slabs (decided when the arguments are read: no GPU needed).
The kernel is held to the twin in test_gpu_output_filter.py."""
import math
import os
import subprocess

import numpy as np
import pytest

from cmc_fluid_solver_amd import build as B
from cmc_fluid_solver_amd import grids
from cmc_fluid_solver_amd import layer_output as LO

HERE = os.path.dirname(os.path.abspath(__file__))
INPUTS = os.path.join(HERE, "golden", "inputs")
DTYPES = [np.float32, np.float64]
DIMS = (9, 8, 7)
SPACING = (0.3, 0.07, 0.11)


def nodes_with_out_block(dims):
    """box_with_obstacle plus a corner block of cells turned NODE_OUT by hand (a coarse box can then hold nothing but NODE_OUT)"""
    n = grids.box_with_obstacle(*dims)
    n.type[:3, :3, :3] = grids.NODE_OUT
    return n


def fields_for(dims, dtype, seed):
    rng = np.random.default_rng(seed)
    return [(rng.standard_normal(dims) * 10.0 ** rng.uniform(-3, 3, dims)).astype(dtype) for _ in range(4)]


def rule_loop(type, fields, outdims, filter, vector, spacing):
    """The rule, cell by cell, in Python scalars of the fields' type"""
    R = fields[0].dtype.type
    g = type.shape
    od = [o or d for o, d in zip(outdims, g)]
    f = [np.array(a, copy=True) for a in fields]
    for a in f:
        a[type == grids.NODE_OUT] = R(99999)
    U, V, W, T = f
    two = [R(2) * R(d) for d in spacing]

    def q(x, y, z):
        ty = type[x, y, z]
        if vector == 0:
            return U[x, y, z], V[x, y, z], W[x, y, z], T[x, y, z]
        if ty == grids.NODE_OUT:
            return R(99999), R(99999), R(99999), T[x, y, z]
        nb = [(x - 1, y, z), (x + 1, y, z), (x, y - 1, z), (x, y + 1, z), (x, y, z - 1), (x, y, z + 1)]
        if ty != grids.NODE_IN or any(not all(0 <= c < d for c, d in zip(p, g)) or type[p] == grids.NODE_OUT for p in nb):
            return R(0), R(0), R(0), T[x, y, z]
        wx = R(R(W[x, y + 1, z] - W[x, y - 1, z]) / two[1]) - R(R(V[x, y, z + 1] - V[x, y, z - 1]) / two[2])
        wy = R(R(U[x, y, z + 1] - U[x, y, z - 1]) / two[2]) - R(R(W[x + 1, y, z] - W[x - 1, y, z]) / two[0])
        wz = R(R(V[x + 1, y, z] - V[x - 1, y, z]) / two[0]) - R(R(U[x, y + 1, z] - U[x, y - 1, z]) / two[1])
        return R(wx), R(wy), R(wz), T[x, y, z]

    def box(i, gg, o):
        lo = i * gg // o
        return lo, max(lo + 1, (i + 1) * gg // o)
    outV = np.empty(od + [3], fields[0].dtype)
    outT = np.empty(od, np.float64)
    for i in range(od[0]):
        for j in range(od[1]):
            for k in range(od[2]):
                (x0, x1), (y0, y1), (z0, z1) = box(i, g[0], od[0]), box(j, g[1], od[1]), box(k, g[2], od[2])
                cells = [(x, y, z) for x in range(x0, x1) for y in range(y0, y1) for z in range(z0, z1) if type[x, y, z] == grids.NODE_IN]
                if filter == 0 or not cells:
                    a, b, c, t = q(x0, y0, z0)
                    outV[i, j, k] = (a, b, c)
                    outT[i, j, k] = float(t)
                    continue
                vals = [q(*p) for p in cells]
                m = [math.fsum(float(v[c]) for v in vals) / float(len(cells)) for c in range(4)]
                outV[i, j, k] = [R(x) for x in m[:3]]
                outT[i, j, k] = m[3]
    return outV, outT


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("filter,vector", [(0, 0), (1, 0), (0, 1), (1, 1)])
def test_twin_equals_a_loop_written_from_the_rule(dtype, filter, vector):
    n = nodes_with_out_block(DIMS)
    fields = fields_for(DIMS, dtype, 5)
    for outdims in ((0, 0, 0), (4, 3, 3), (1, 1, 1), (12, 3, 9)):
        V, T = LO.layer_output(n.type, fields, outdims, filter, vector, SPACING, exact_sum=True)
        eV, eT = rule_loop(n.type, fields, outdims, filter, vector, SPACING)
        assert V.dtype == np.dtype(dtype) and T.dtype == np.float64
        assert np.array_equal(V, eV) and np.array_equal(T, eT), (outdims, filter, vector)
        # numpy's own double sum stays within the rounding of a sum of n terms of the exact one
        V2, T2 = LO.layer_output(n.type, fields, outdims, filter, vector, SPACING)
        assert np.allclose(T2, T, rtol=0, atol=1e-9) and np.allclose(V2, V, rtol=1e-6, atol=1e-6)


def test_boxes_partition_an_axis_and_start_at_the_sample_cell():
    for g in (1, 2, 7, 10, 11, 70, 130, 256):
        for o in list(range(1, g + 1)) + [0]:
            lo, hi = LO.boxes(g, o)
            n = o or g
            assert lo[0] == 0 and hi[-1] == g and np.array_equal(hi[:-1], lo[1:]) and (hi > lo).all()
            assert np.array_equal(lo, np.arange(n) * g // n)
        for o in (g, g + 1, 2 * g + 3, 50 * g):
            lo, hi = LO.boxes(g, o)
            assert np.array_equal(hi, lo + 1) and np.array_equal(lo, np.arange(o) * g // o)
    g, o = (1 << 31) - 1, 1000                             # 64-bit products
    lo, hi = LO.boxes(g, o)
    assert [int(v) for v in lo] == [i * g // o for i in range(o)] and int(hi[-1]) == g


@pytest.mark.parametrize("dtype", DTYPES)
def test_box_filter_on_single_cell_boxes_is_the_gather(dtype):
    n = nodes_with_out_block(DIMS)
    fields = fields_for(DIMS, dtype, 6)
    st = LO.stamp(n.type, fields)
    for outdims in ((0, 0, 0), DIMS, (20, 8, 15)):
        od = [o or d for o, d in zip(outdims, DIMS)]
        sel = np.ix_(*[np.arange(o) * d // o for o, d in zip(od, DIMS)])
        eV, eT = np.stack([f[sel] for f in st[:3]], axis=-1), st[3][sel].astype(np.float64)
        for filter in (0, 1):
            V, T = LO.layer_output(n.type, fields, outdims, filter)
            assert np.array_equal(V, eV) and np.array_equal(T, eT), (outdims, filter)
        for a, b in zip(LO.layer_output(n.type, fields, outdims, 0, 1, SPACING), LO.layer_output(n.type, fields, outdims, 1, 1, SPACING)):
            assert np.array_equal(a, b), outdims
    assert all(np.array_equal(a, b) for a, b in zip(fields, fields_for(DIMS, dtype, 6))), "the fields are not modified"


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_constant_fluid_field_comes_out_as_the_constant(dtype):
    n = nodes_with_out_block((13, 11, 10))
    fluid = n.type == grids.NODE_IN
    # fp32: n * (double)c is exact for every c (24 + 29 bits), so any constant comes back.  fp64: that holds for constants of few
    # significant bits only -- the sum of n copies of 0.1 is rounded, and the mean is 0.1 to that rounding, not bit for bit
    consts = [dtype(c) for c in ((0.1, -3.3, 1e-3, 291.7) if dtype == np.float32 else (0.125, -3.25, 2.0 ** -10, 291.75))]
    fields = fields_for(n.shape, dtype, 7)
    for f, c in zip(fields, consts):
        f[fluid] = c
    od = (5, 4, 3)
    V, T = LO.layer_output(n.type, fields, od, LO.BOX)
    has_fluid = LO.box_kinds(n.type, od) <= 1
    assert has_fluid.any() and not has_fluid.all()
    for c in range(3):
        assert (V[..., c][has_fluid] == consts[c]).all()
    assert (T[has_fluid] == float(consts[3])).all()


@pytest.mark.parametrize("dtype", DTYPES)
def test_curl_of_a_rigid_rotation_is_exact_on_power_of_two_spacings(dtype):
    n = nodes_with_out_block((13, 11, 10))
    sp = (0.25, 0.125, 0.5)
    x, y, _ = np.meshgrid(*[np.arange(d) * h for d, h in zip(n.shape, sp)], indexing="ij")
    fields = [(-y).astype(dtype), x.astype(dtype), np.zeros(n.shape, dtype), np.ones(n.shape, dtype)]
    V, T = LO.layer_output(n.type, fields, (0, 0, 0), LO.POINT, LO.VORTICITY, sp)
    ok = LO.curl_defined(n.type)
    out_cells = n.type == grids.NODE_OUT
    assert ok.any() and (ok <= (n.type == grids.NODE_IN)).all()
    beside_out = (n.type == grids.NODE_IN) & ~ok
    assert beside_out.any(), "a fluid cell beside a NODE_OUT cell carries no curl"
    assert np.array_equal(V[ok], np.broadcast_to(np.array([0, 0, 2], dtype), V[ok].shape))
    assert (V[out_cells] == 99999).all() and (T[out_cells] == 99999.0).all()
    assert (V[~ok & ~out_cells] == 0).all()
    # the box mean of it: 2 times the share of the box's fluid cells that carry a curl
    od = (4, 3, 3)
    bV, _ = LO.layer_output(n.type, fields, od, LO.BOX, LO.VORTICITY, sp, exact_sum=True)
    kinds = LO.box_kinds(n.type, od)
    for (i, j, k), kind in np.ndenumerate(kinds):
        box = tuple(slice(lo[a], hi[a]) for a, (lo, hi) in zip((i, j, k), [LO.boxes(g, o) for g, o in zip(n.shape, od)]))
        fl = n.type[box] == grids.NODE_IN
        if kind <= 1:
            assert bV[i, j, k, 2] == dtype(2.0 * ok[box].sum() / fl.sum()) and bV[i, j, k, 0] == 0 and bV[i, j, k, 1] == 0
        else:
            assert (bV[i, j, k] == (99999 if kind == 3 else 0)).all()


def test_bad_arguments_are_refused():
    n = grids.box(5, 5, 5)
    f = fields_for(n.shape, np.float32, 1)
    with pytest.raises(ValueError):
        LO.layer_output(n.type, f, (0, 0, 0), 2)
    with pytest.raises(ValueError):
        LO.layer_output(n.type, f, (0, 0, 0), 0, 2, SPACING)
    with pytest.raises(ValueError):
        LO.layer_output(n.type, f, (0, 0, 0), 0, 1)          # the curl needs the spacing


def test_driver_refuses_the_box_filter_on_slabs_when_it_reads_the_arguments(built, tmp_path):
    driver = B.build_driver()
    data, cfgf = (os.path.join(INPUTS, f) for f in ("box_pipe_2D_data.txt", "box_pipe_2D_config.txt"))
    prefix = str(tmp_path / "o")
    r = subprocess.run([driver, data, prefix, cfgf, "align", "GPU", "2", "--same-device", "--output-filter", "box"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "--output-filter box: single GPU only" in r.stderr and "x-slabs" in r.stderr
    assert "Grid =" not in r.stdout and not os.path.exists(prefix + "_res.nc"), "refused before the geometry is loaded"
    r = subprocess.run([driver, data, prefix, cfgf, "align", "GPU", "--output-filter", "tent"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "--output-filter: point or box" in r.stderr
    assert "[--output-filter point|box]" in subprocess.run([driver], capture_output=True, text=True, timeout=60).stdout
