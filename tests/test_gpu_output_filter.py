"""Filtered and derived result records on the device (k_get_layer_box, csrc/kernels_output.hip, behind FS3D_OPT_OUTPUT_FILTER / FS3D_OPT_OUTPUT_VECTOR)
against the rule's numpy twin, cmc_fluid_solver_amd/layer_output.py.

Exact fields (integers + 0.5 below 2^23, all different): every double sum is exact whatever order the kernel adds in, so the
comparison is array_equal.  General fields (normal values scaled over 1e-3 .. 1e3): the bound is derived, not measured -- for a
sample with n = |C| fluid cells and A = sum |q| over them, against m* = fsum(q) / n (one rounding in the sum, one in the division):
  a double sum of n terms in any order is within (n - 1) * 2^-53 * A of the exact sum (to first order), fsum within 2^-53 * A,
  and each of the two divisions adds 2^-53 of its quotient, at most 2^-53 * A / n:   |outT - m*| <= (n + 2) * 2^-53 * A / n;
  outV is that mean rounded once to R:                                            |outV - m*| <= the same + eps_R * |m*|,
with eps_R = 2^-24 in fp32 and 2^-53 in fp64.  Samples whose box holds no fluid are point samples: array_equal."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

from cmc_fluid_solver_amd import build as B
from cmc_fluid_solver_amd import capi, grids, shape2d
from cmc_fluid_solver_amd import layer_output as LO
from cmc_fluid_solver_amd.slab import slab_range

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
INPUTS = os.path.join(HERE, "golden", "inputs")
PARAMS = (200.0, 0.72, 1.4)
DTYPES = [np.float32, np.float64]
GRIDS = [(13, 11, 10), (23, 13, 11), (9, 7, 70), (6, 5, 130)]       # dimz % 4 != 0; more than one wave along k; more than two
POW2 = (0.25, 0.125, 0.5)
GENERAL = (0.3, 0.07, 0.11)
MODES = [(1, 0), (0, 1), (1, 1)]                                    # (filter, vector); (0, 0) is the default path
COARSE = (5, 4, 7)


@pytest.fixture(scope="module", autouse=True)
def _torch_first():
    import torch
    torch.cuda.init()                    # before the library opens the device


def outdims_of(dims):
    return [(0, 0, 0), (1, 1, 1), (4, 3, 3), COARSE, (50, 3, 4), (dims[0], 5, dims[2])]


def make_nodes(dims, spacing, out_block=True):
    """A box with an obstacle and, by hand, a corner block of NODE_OUT cells: fluid cells beside NODE_OUT cells, and coarse boxes
    that hold nothing but NODE_OUT"""
    n = grids.box_with_obstacle(*dims)
    n.dx, n.dy, n.dz = spacing
    # on the thinnest grid the obstacle is one cell thick: a wall cell between two fluid runs, which the library takes with a
    # no-slip temperature condition only (no test here steps these grids, so the condition changes no result)
    inside = np.zeros(n.shape, bool)
    inside[1:-1, 1:-1, 1:-1] = True
    n.bc_temp[inside & (n.type == grids.NODE_BOUND)] = grids.BC_NOSLIP
    if out_block:
        n.type[:3, :3, :3] = grids.NODE_OUT
    return n


def exact_fields(shape, dtype, seed):
    """Four fields whose 4*n values are all different (integers + 0.5, exact in fp32 up to 2^23), in a random order."""
    n = int(np.prod(shape))
    assert 4 * n < 1 << 23
    perm = np.random.default_rng(seed).permutation(4 * n)
    return [(perm[v * n:(v + 1) * n] + 0.5).astype(dtype).reshape(shape) for v in range(4)]


def general_fields(shape, dtype, seed):
    rng = np.random.default_rng(seed)
    return [(rng.standard_normal(shape) * 10.0 ** rng.uniform(-3, 3, shape)).astype(dtype) for _ in range(4)]


def solver_with_next(nodes, dtype, fields):
    s = capi.Solver(nodes, capi.fluid_params(dtype, *PARAMS), dtype)
    s.upload_layer(capi.LAYER_NEXT, fields)
    return s


def set_mode(s, filter, vector):
    s.set_option(capi.OPT_OUTPUT_FILTER, filter)
    s.set_option(capi.OPT_OUTPUT_VECTOR, vector)


def nan_arrays(od, dtype):
    return np.full(tuple(od) + (3,), np.nan, dtype), np.full(tuple(od), np.nan, np.float64)


def assert_within_bound(type, fields, outdims, vector, spacing, V, T, what):
    """The derived bound of the module docstring, sample by sample; prints the largest share of it that was used."""
    type = np.asarray(type)
    q = LO.cell_quantities(type, fields, vector, spacing)
    eV, eT = LO.layer_output(type, fields, outdims, LO.BOX, vector, spacing, exact_sum=True)
    eps = 2.0 ** -24 if q[0].dtype == np.float32 else 2.0 ** -53
    ax = [LO.boxes(g, o) for g, o in zip(type.shape, outdims)]
    used = 0.0
    for i, (x0, x1) in enumerate(zip(*ax[0])):
        for j, (y0, y1) in enumerate(zip(*ax[1])):
            for k, (z0, z1) in enumerate(zip(*ax[2])):
                box = (slice(x0, x1), slice(y0, y1), slice(z0, z1))
                m = type[box] == grids.NODE_IN
                n = int(m.sum())
                if n == 0:
                    assert np.array_equal(V[i, j, k], eV[i, j, k]) and T[i, j, k] == eT[i, j, k], (what, i, j, k)
                    continue
                for c in range(4):
                    A = math.fsum(np.abs(q[c][box][m].astype(np.float64)))
                    got, want = (float(V[i, j, k, c]), float(eV[i, j, k, c])) if c < 3 else (T[i, j, k], eT[i, j, k])
                    mstar = math.fsum(q[c][box][m].astype(np.float64)) / n
                    bound = (n + 2) * 2.0 ** -53 * A / n + (eps * abs(mstar) if c < 3 else 0.0)
                    err = abs(got - mstar)
                    assert err <= bound, (what, (i, j, k), c, n, err, bound)
                    if bound > 0:
                        used = max(used, err / bound)
    print("%s: largest error / bound = %.3f" % (what, used))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("dims", GRIDS)
def test_exact_fields_equal_the_twin_bit_for_bit(built, dims, dtype):
    nodes = make_nodes(dims, POW2)
    kinds = LO.box_kinds(nodes.type, COARSE)
    assert [int((kinds == v).sum()) > 0 for v in range(4)] == [True] * 4, "all fluid, mixed, no fluid on a wall, no fluid on NODE_OUT"
    fields = exact_fields(dims, dtype, 11)
    s = solver_with_next(nodes, dtype, fields)
    for outdims in outdims_of(dims):
        for filter, vector in MODES:
            set_mode(s, filter, vector)
            V, T = s.GetLayer(outdims)
            eV, eT = LO.layer_output(nodes.type, fields, outdims, filter, vector, POW2)
            assert V.dtype == np.dtype(dtype) and np.array_equal(V, eV) and np.array_equal(T, eT), (outdims, filter, vector)
    s.close()


LONG = [((3, 3, 600), [(0, 0, 0), (1, 1, 1), (3, 3, 2), (3, 3, 3), (2, 2, 300), (1, 1, 599)]),
        ((3, 4, 777), [(0, 0, 0), (1, 1, 1), (3, 4, 2), (3, 4, 3), (2, 2, 600), (1, 1, 259)])]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("dims,outdims_list", LONG)
def test_lines_longer_than_the_block_equal_the_twin_bit_for_bit(built, dims, outdims_list, dtype):
    """The kernel walks a source line in chunks of 256 cells and takes the output k in groups of 256.  Lines of 600 and 777 cells:
    odz 1, 2, 3 -- boxes wider than a chunk, which accumulate over chunks, and box edges (300; 259, 518) inside a chunk; odz 300, 599,
    600, 777 and 259 -- two to four groups of output k, their source ranges starting inside a chunk.  The line through the middle of
    these thin boxes is the fluid; a run of it is turned NODE_OUT by hand, across a chunk edge."""
    nodes = grids.box(*dims)
    nodes.dx, nodes.dy, nodes.dz = POW2
    nodes.type[1, 1, 250:262] = grids.NODE_OUT
    fluid = nodes.type == grids.NODE_IN
    assert fluid[1, 1, 1:250].all() and fluid[1, 1, 262:-1].all() and fluid.sum() >= dims[2] - 14
    fields = exact_fields(dims, dtype, 19)
    s = solver_with_next(nodes, dtype, fields)
    for outdims in outdims_list:
        for filter, vector in MODES:
            set_mode(s, filter, vector)
            V, T = s.GetLayer(outdims)
            eV, eT = LO.layer_output(nodes.type, fields, outdims, filter, vector, POW2)
            assert np.array_equal(V, eV) and np.array_equal(T, eT), (outdims, filter, vector)
        if outdims[2] in (2, 3):                           # the boxes that span chunks hold fluid, a wall and the outside
            assert (LO.box_kinds(nodes.type, outdims) == 1).any()
    s.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_single_cell_boxes_equal_the_point_sample_through_all_three_entries(built, dtype):
    import torch
    dims = GRIDS[0]
    nodes = make_nodes(dims, GENERAL)
    fields = general_fields(dims, dtype, 12)
    s = solver_with_next(nodes, dtype, fields)
    td = torch.float32 if dtype == np.float32 else torch.float64
    for outdims in ((0, 0, 0), dims, (20, 11, 15)):
        od = tuple(o or d for o, d in zip(outdims, dims))
        for vector in (0, 1):
            res = {}
            for filter in (0, 1):
                set_mode(s, filter, vector)
                gV, gT = s.GetLayer(outdims)
                rV, rT = nan_arrays(od, dtype)
                assert s.GetLayerRows(rV, rT, outdims) == (0, od[0])
                dV = torch.full(od + (3,), -7.0, dtype=td, device="cuda")
                dT = torch.full(od, -7.0, dtype=torch.float64, device="cuda")
                torch.cuda.synchronize()
                assert s.GetLayerDev(dV, dT, outdims) == (0, od[0])
                s.synchronize()
                for a, b in ((rV, rT), (dV.cpu().numpy(), dT.cpu().numpy())):
                    assert np.array_equal(a, gV) and np.array_equal(b, gT), (outdims, filter, vector)
                res[filter] = (gV, gT)
            assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1]), (outdims, vector)
            eV, eT = LO.layer_output(nodes.type, fields, outdims, 0, vector, GENERAL)
            assert np.array_equal(res[0][0], eV) and np.array_equal(res[0][1], eT), (outdims, vector)
    s.close()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("dims", [(23, 13, 11), (9, 7, 70)])
def test_general_fields_stay_within_the_derived_bound(built, dims, dtype):
    nodes = make_nodes(dims, GENERAL)
    fields = general_fields(dims, dtype, 13)
    s = solver_with_next(nodes, dtype, fields)
    for outdims in ((1, 1, 1), (4, 3, 3), COARSE):
        for vector in (0, 1):                              # vector 1: general spacings, q the curl
            set_mode(s, 1, vector)
            V, T = s.GetLayer(outdims)
            assert_within_bound(nodes.type, fields, outdims, vector, GENERAL, V, T, "%s %s %s vector %d" % (dims, np.dtype(dtype).name, outdims, vector))
    s.close()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("dims", [(13, 11, 10), (6, 5, 130)])
def test_point_vorticity_equals_the_twin_on_general_spacings(built, dims, dtype):
    nodes = make_nodes(dims, GENERAL)
    ok = LO.curl_defined(nodes.type)
    fluid = nodes.type == grids.NODE_IN
    assert (fluid & ~ok).any() and not ok[0].any() and not ok[:, :, -1].any(), "fluid beside NODE_OUT, and the faces, carry no curl"
    fields = general_fields(dims, dtype, 14)
    s = solver_with_next(nodes, dtype, fields)
    set_mode(s, 0, 1)
    for outdims in ((0, 0, 0), COARSE, (50, 3, 4)):
        V, T = s.GetLayer(outdims)
        eV, eT = LO.layer_output(nodes.type, fields, outdims, 0, 1, GENERAL)
        assert np.array_equal(V, eV) and np.array_equal(T, eT), outdims
        if outdims == (0, 0, 0):
            out_cells = nodes.type == grids.NODE_OUT
            assert (V[out_cells] == 99999).all() and (V[fluid & ~ok] == 0).all() and (V[ok] != 0).any()
            assert (V[0] == np.where(out_cells[0][..., None], 99999, 0)).all(), "the x = 0 face"
        else:
            assert (V[0, 0, 0] == 99999).all(), "a NODE_OUT sample"
    s.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_call_leaves_the_state_a_default_call_leaves(built, dtype):
    import torch
    dims = GRIDS[1]
    nodes = make_nodes(dims, GENERAL)
    fields, cur = exact_fields(dims, dtype, 15), general_fields(dims, dtype, 16)
    ref = solver_with_next(nodes, dtype, fields)
    dV, dT = ref.GetLayer(COARSE)
    ref_next, ref_info = ref.download_layer(capi.LAYER_NEXT), ref.get_layer_info()
    ref.close()
    s = solver_with_next(nodes, dtype, fields)
    s.upload_layer(capi.LAYER_CUR, cur)
    for filter, vector in MODES:
        set_mode(s, filter, vector)
        V, T = s.GetLayer(COARSE)
        eV, eT = LO.layer_output(nodes.type, fields, COARSE, filter, vector, GENERAL, exact_sum=True)
        if vector == 0:
            assert np.array_equal(V, eV) and np.array_equal(T, eT)
        assert all(np.array_equal(a, b) for a, b in zip(s.download_layer(capi.LAYER_NEXT), ref_next)), "next: the stamp and nothing else"
        assert all(np.array_equal(a, b) for a, b in zip(s.download_layer(capi.LAYER_CUR), cur)), "cur is untouched"
        assert s.get_layer_info() == ref_info
        rV, rT = nan_arrays(COARSE, dtype)
        assert s.GetLayerRows(rV, rT, COARSE) == (0, COARSE[0])
        assert np.array_equal(rV, V) and np.array_equal(rT, T) and s.get_layer_info() == ref_info
        gV = torch.full(COARSE + (3,), -7.0, dtype=torch.float32 if dtype == np.float32 else torch.float64, device="cuda")
        gT = torch.full(COARSE, -7.0, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        assert s.GetLayerDev(gV, gT, COARSE) == (0, COARSE[0])
        s.synchronize()
        assert np.array_equal(gV.cpu().numpy(), V) and np.array_equal(gT.cpu().numpy(), T), "the device destination gets the same box means"
        info = s.get_layer_info()
        assert info["samples"] == ref_info["samples"] and info["bytes_to_host"] == 0
    set_mode(s, 0, 0)
    V, T = s.GetLayer(COARSE)
    assert np.array_equal(V, dV) and np.array_equal(T, dT), "both options back to 0: the default record"
    s.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_geometry_update_is_seen_by_the_next_record(built, dtype):
    dims = GRIDS[1]
    nodes = make_nodes(dims, POW2, out_block=False)
    moved = grids.box_with_obstacle(*dims, lo=0.2, hi=0.5)
    moved.dx, moved.dy, moved.dz = POW2
    assert (nodes.type != moved.type).any()
    fields = exact_fields(dims, dtype, 17)
    s = solver_with_next(nodes, dtype, fields)
    set_mode(s, 1, 1)
    s.GetLayer(COARSE)
    s.update_nodes(moved)
    s.upload_layer(capi.LAYER_NEXT, fields)
    for filter, vector in MODES:
        set_mode(s, filter, vector)
        V, T = s.GetLayer(COARSE)
        eV, eT = LO.layer_output(moved.type, fields, COARSE, filter, vector, POW2)
        oV, _ = LO.layer_output(nodes.type, fields, COARSE, filter, vector, POW2)
        assert np.array_equal(V, eV) and np.array_equal(T, eT) and not np.array_equal(V, oV), (filter, vector)
    s.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_record_after_two_time_steps(built, dtype):
    dims = GRIDS[1]
    nodes = grids.box_with_obstacle(*dims)
    spacing = (nodes.dx, nodes.dy, nodes.dz)
    s = capi.Solver(nodes, capi.fluid_params(dtype, *PARAMS), dtype)
    for _ in range(2):
        s.UpdateBoundaries()
        s.TimeStep(dtype(0.05), 2, 1, True)
    for vector in (0, 1):
        set_mode(s, 1, vector)
        V, T = s.GetLayer(COARSE)
        after = s.download_layer(capi.LAYER_NEXT)
        assert any(np.abs(f[nodes.type == grids.NODE_IN]).max() > 0 for f in after[:3])
        assert_within_bound(nodes.type, after, COARSE, vector, spacing, V, T, "two steps %s vector %d" % (np.dtype(dtype).name, vector))
    s.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_refusals(built, dtype):
    dims = GRIDS[1]
    nodes = make_nodes(dims, GENERAL, out_block=False)
    fields = exact_fields(dims, dtype, 18)
    params = capi.fluid_params(dtype, *PARAMS)
    one = solver_with_next(nodes, dtype, fields)
    for opt in (capi.OPT_OUTPUT_FILTER, capi.OPT_OUTPUT_VECTOR):
        for bad in (2, -1):
            assert one.lib.fs3d_set_option(one.h, opt, bad) == capi.ERR_INVALID
    eV, eT = LO.layer_output(nodes.type, fields, COARSE)
    V, T = one.GetLayer(COARSE)
    assert np.array_equal(V, eV) and np.array_equal(T, eT), "a refused value leaves the option as it was"
    one.close()
    grp = capi.LocalGroup(nodes, params, 2, dtype)
    lone = capi.Solver(nodes, params, dtype, x_range=(5, 17))
    ctxs = grp.solvers + [lone]
    for s in ctxs:
        s.upload_layer(capi.LAYER_NEXT, [f[s.x0:s.x1] for f in fields])
    rows = (C.c_int * 2)(-1, -1)
    for filter, vector in MODES:
        for s in ctxs:
            set_mode(s, filter, vector)
            before = s.download_layer(capi.LAYER_NEXT)
            V, T = nan_arrays(COARSE, dtype)
            pV, pT = V.ctypes.data_as(C.c_void_p), T.ctypes.data_as(C.c_void_p)
            assert s.lib.fs3d_get_layer(s.h, pV, pT, *COARSE) == capi.ERR_UNSUPPORTED
            assert b"x-slab" in s.lib.fs3d_last_error(s.h)
            assert s.lib.fs3d_get_layer_rows(s.h, pV, pT, *COARSE, rows) == capi.ERR_UNSUPPORTED
            assert s.lib.fs3d_get_layer_dev(s.h, pV, pT, *COARSE, rows) == capi.ERR_UNSUPPORTED      # refused before the pointers are used
            assert np.isnan(V).all() and np.isnan(T).all() and list(rows) == [-1, -1]
            assert all(np.array_equal(a, b) for a, b in zip(s.download_layer(capi.LAYER_NEXT), before)), "no stamp either"
    # both options 0: the slabs sample as they always did
    st = LO.stamp(nodes.type, fields)
    for s in ctxs:
        set_mode(s, 0, 0)
        V, T = s.GetLayer(COARSE)
        eV, eT = LO.layer_output(nodes.type[s.x0:s.x1], [f[s.x0:s.x1] for f in fields], COARSE)
        assert np.array_equal(V, eV) and np.array_equal(T, eT)
        gV, gT = nan_arrays(COARSE, dtype)
        i0, i1 = s.GetLayerRows(gV, gT, COARSE)
        gx = np.arange(i0, i1) * dims[0] // COARSE[0]
        sel = np.ix_(gx, np.arange(COARSE[1]) * dims[1] // COARSE[1], np.arange(COARSE[2]) * dims[2] // COARSE[2])
        assert np.array_equal(gV[i0:i1], np.stack([f[sel] for f in st[:3]], axis=-1)) and np.array_equal(gT[i0:i1], st[3][sel].astype(np.float64))
    lone.close()
    grp.close()


def _driver_case(tmp_path, out_grid=None):
    data, cfgf = (os.path.join(INPUTS, f) for f in ("box_pipe_2D_data.txt", "box_pipe_2D_config.txt"))
    if out_grid is not None:
        text = open(cfgf).read()
        for name, v in zip(("out_gridx", "out_gridy", "out_gridz"), out_grid):
            line = [l for l in text.splitlines() if l.split() and l.split()[0] == name]
            assert len(line) == 1
            text = text.replace(line[0], "%s\t%d" % (name, v))
        cfgf = str(tmp_path / "config.txt")
        open(cfgf, "w").write(text)
    return data, cfgf


def test_driver_box_word_on_a_full_resolution_output_writes_the_same_bytes(built, tmp_path, monkeypatch):
    monkeypatch.setenv("FS3D_DEFAULT_KERNEL", "4")
    driver = B.build_driver()
    # box_pipe is a 64^3 grid and its shipped config samples 54 x 54 x 52 of it, as every shipped config samples fewer cells than
    # its grid has: the config here is the shipped one with an output grid at least as fine as the grid on every axis
    data, cfgf = _driver_case(tmp_path, (70, 64, 66))
    nodes, cfg, _ = shape2d.load_case(data, cfgf, align=True)
    assert all(o >= d for o, d in zip((cfg.outdimx, cfg.outdimy, cfg.outdimz), nodes.shape)), "every box is one cell"
    files = []
    for tag, words in (("point", []), ("box", ["--output-filter", "box"]), ("word", ["--output-filter", "point"])):
        prefix = str(tmp_path / tag)
        subprocess.run([driver, data, prefix, cfgf, "align", "GPU", "--steps", "11"] + words, check=True, capture_output=True, text=True, timeout=300)
        files.append(open(prefix + "_res.nc", "rb").read())
    assert len(files[0]) > 1000 and files[0] == files[1] == files[2]


def test_driver_box_word_on_a_coarse_output_writes_the_twins_records(built, tmp_path, monkeypatch):
    from scipy.io import netcdf_file
    monkeypatch.setenv("FS3D_DEFAULT_KERNEL", "4")
    driver = B.build_driver()
    od = (7, 6, 5)
    data, cfgf = _driver_case(tmp_path, od)
    nsteps = 11
    prefix = str(tmp_path / "box")
    subprocess.run([driver, data, prefix, cfgf, "align", "GPU", "--steps", str(nsteps), "--output-filter", "box"], check=True, capture_output=True,
                   text=True, timeout=300)
    nodes, cfg, dt = shape2d.load_case(data, cfgf, align=True)
    assert (cfg.outdimx, cfg.outdimy, cfg.outdimz) == od
    s = capi.Solver(nodes, capi.fluid_params(np.float32, cfg.Re, cfg.Pr, cfg.lam), np.float32)
    layers = []
    for i in range(nsteps):
        s.UpdateBoundaries()
        s.TimeStep(np.float32(dt), cfg.num_global, cfg.num_local, i % 10 == 0)
        if i % cfg.out_time_steps == 0:
            s.GetLayer(od)                                 # the driver's call: the stamp
            layers.append(s.download_layer(capi.LAYER_NEXT))
    s.close()
    f = netcdf_file(prefix + "_res.nc", "r", mmap=False)
    assert f.variables["u"].shape == (len(layers),) + od and len(layers) == 2
    point_differs = False
    for r, fields in enumerate(layers):
        V = np.stack([np.asarray(f.variables[nm][r], np.float64) for nm in "uvw"], axis=-1)
        T = np.ascontiguousarray(f.variables["T"][r], np.float64)
        assert np.array_equal(V, V.astype(np.float32)), "the file holds the library's fp32 samples"
        assert_within_bound(nodes.type, fields, od, 0, None, V.astype(np.float32), T, "driver record %d" % r)
        point_differs = point_differs or not np.array_equal(V.astype(np.float32), LO.layer_output(nodes.type, fields, od)[0])
    f.close()
    assert point_differs, "the box mean is not the point sample on this output grid"
