"""GPU: the gradient sums of the time statistics (FS3D_OPT_TIME_STATS_GRAD: k_time_grad, csrc/kernels_stats.hip) and their read-out
(FS3D_OPT_OUTPUT_GRADIENT 2: k_time_grad_layer) against the numpy twin, time_stats.TimeStats(gradients=True).

As in test_gpu_time_stats.py the twin is fed the `cur` downloaded after each step of the same context, so the rounding of the
sweeps plays no part.  The sums are per cell, in step order, in double, and the invariants are the twin's bit for bit: the
full-resolution record is array_equal; through the box filter it stays inside the derived bound of test_gpu_output_filter.py.
A step is `real` (UpdateBoundaries, one ADI step), `fresh` (a random `cur` near the node values uploaded first, then real) or
`swap` (general fields over 1e-3 .. 1e3 uploaded into `next`, then a step of zero iterations, which only swaps).  The grids that
the sweeps' tables were never asked to step (a block one cell thick, lines of one cell) take `swap` steps only.
Every test sets option 21 first: on a library without the option each of them fails there."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

from test_gpu_output_filter import assert_within_bound, general_fields, make_nodes, nan_arrays  # noqa: E402
from test_gpu_time_stats import gather, near_one, same  # noqa: E402
from cmc_fluid_solver_amd import build as B  # noqa: E402
from cmc_fluid_solver_amd import capi, grids, shape2d  # noqa: E402
from cmc_fluid_solver_amd import layer_output as LO  # noqa: E402
from cmc_fluid_solver_amd import time_stats as TS  # noqa: E402

pytestmark = pytest.mark.gpu

PARAMS = (200.0, 0.72, 1.4)
DT = 0.1
DTYPES = [np.float32, np.float64]
COARSE = (5, 4, 7)
GENERAL = (0.3, 0.07, 0.11)
# (grid, plan): dimz % 4 != 0 with real steps; more than one wave along k; more than two; one interior row and a k range past 256;
# one defined cell
CASES = [((13, 11, 10), ("real", "swap", "fresh", "real", "swap")), ((9, 7, 70), ("swap",) * 4), ((6, 5, 130), ("swap",) * 3),
         ((4, 3, 261), ("swap",) * 4), ((3, 3, 3), ("swap",) * 3)]
IDS = ["x".join(map(str, c[0])) for c in CASES]


@pytest.fixture(scope="module", autouse=True)
def _torch_first():
    import torch
    torch.cuda.init()                    # before the library opens the device


def geometries(dims):
    """(A, B): the geometry of the window and one that turns cells which carry invariants in A into walls or the outside"""
    if dims == (13, 11, 10):
        A, Bg = grids.box_with_obstacle(*dims, lo=0.25, hi=0.55), grids.box_with_obstacle(*dims, lo=0.45, hi=0.75)
    elif dims in ((9, 7, 70), (6, 5, 130)):
        A, Bg = make_nodes(dims, GENERAL, out_block=False), make_nodes(dims, GENERAL)
        if dims == (9, 7, 70):
            # NODE_OUT by hand either side of the edge between the first two waves of 64 lanes, in two fluid rows: the cell at k = 63
            # (last lane of its wave) loses its invariants to the type at k + 1, the cell at k = 64 (first lane) to the type at k - 1
            fluid = np.asarray(A.type) == grids.NODE_IN
            rows = [(x, y) for x in range(1, dims[0] - 1) for y in range(1, dims[1] - 1) if fluid[x - 1:x + 2, y - 1:y + 2, 61:67].all()]
            assert len(rows) >= 2 and LO.curl_defined(A.type)[rows[0] + (63,)] and LO.curl_defined(A.type)[rows[-1] + (64,)]
            Bg.type[rows[0] + (64,)] = grids.NODE_OUT
            Bg.type[rows[-1] + (63,)] = grids.NODE_OUT
            okB = LO.curl_defined(Bg.type)
            assert not okB[rows[0] + (63,)] and not okB[rows[-1] + (64,)] and okB[rows[0] + (62,)] and okB[rows[-1] + (65,)]
    else:
        A, Bg = grids.box(*dims), grids.box(*dims)
        if dims == (4, 3, 261):
            Bg.type[1, 1, 250:262] = grids.NODE_OUT                 # across the edge of the first chunk of 256 lanes
    for n in (A, Bg):
        n.dx, n.dy, n.dz = GENERAL
    return A, Bg


def do_step(s, kind, rng, nodes, seed):
    if kind == "swap":
        s.upload_layer(capi.LAYER_NEXT, general_fields(s.dims, s.dtype.type, seed))
        s.TimeStep(DT, 0, 0, False)
    else:
        if kind == "fresh":
            s.upload_layer(capi.LAYER_CUR, near_one(rng, s.dims, s.dtype, nodes))
        s.UpdateBoundaries()
        s.TimeStep(DT, 1, 1, False)
    return s.download_layer(capi.LAYER_CUR)


def expected(twin, cur, types, od):
    return gather(LO.stamp(types, twin.gradient_layer(cur)), od)


def check_record(s, twin, types, what):
    """FS3D_OPT_OUTPUT_GRADIENT 2 at full resolution and through the gather: array_equal; through the box filter: the bound"""
    cur = s.download_layer(capi.LAYER_CUR)
    s.set_option(capi.OPT_OUTPUT_SOURCE, 1)
    s.set_option(capi.OPT_OUTPUT_GRADIENT, 2)
    for outdims in ((0, 0, 0), COARSE):
        od = tuple(o or d for o, d in zip(outdims, s.dims))
        V, T = s.GetLayer(outdims)
        eV, eT = expected(twin, cur, types, od)
        assert same(V, eV) and same(T, eT), (what, outdims)
    s.set_option(capi.OPT_OUTPUT_FILTER, 1)
    V, T = s.GetLayer(COARSE)
    assert_within_bound(types, twin.gradient_layer(cur), COARSE, LO.VELOCITY, None, V, T, "%s box mean" % (what,))
    for opt in (capi.OPT_OUTPUT_FILTER, capi.OPT_OUTPUT_GRADIENT, capi.OPT_OUTPUT_SOURCE):
        s.set_option(opt, 0)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("every", [1, 2])
@pytest.mark.parametrize("dims,plan", CASES, ids=IDS)
def test_gradient_sums_equal_the_twin_with_a_geometry_that_moves(built, dims, plan, every, dtype):
    A, Bg = geometries(dims)
    tA, tB = np.asarray(A.type), np.asarray(Bg.type)
    moves = (tA != tB).any()
    assert moves == (dims != (3, 3, 3)) and LO.curl_defined(tA).any()
    if moves:
        assert (LO.curl_defined(tA) & ~LO.curl_defined(tB)).any()
    s = capi.Solver(A, capi.fluid_params(dtype, *PARAMS), dtype)
    s.set_option(capi.OPT_TIME_STATS, 1)
    s.set_option(capi.OPT_TIME_STATS_EVERY, every)
    s.set_option(capi.OPT_TIME_STATS_GRAD, 1)
    twin = TS.TimeStats(dims, 1, every=every, gradients=True, spacing=GENERAL)
    rng = np.random.default_rng(41)
    for k, kind in enumerate(plan):
        nodes = Bg if k in (1, 2) else A                            # A, B, B, A, ..: cells lose their invariants and get them back
        if moves and k in (1, 3):
            s.update_nodes(nodes)
        twin.add(do_step(s, kind, rng, nodes, 50 + k), np.asarray(nodes.type))
    assert twin.N == (len(plan) + every - 1) // every and twin.ng.max() == twin.N
    if moves and every == 1:
        assert (twin.ng[twin.ng > 0] < twin.N).any(), "cells that carried invariants on some steps only"
    check_record(s, twin, np.asarray(nodes.type), "%s every %d" % (dims, every))
    # the record of the fields is what it is without the option
    s.set_option(capi.OPT_OUTPUT_SOURCE, 1)
    V, T = s.GetLayer(COARSE)
    eV, eT = gather(LO.stamp(np.asarray(nodes.type), twin.layer(1, s.download_layer(capi.LAYER_CUR))), COARSE)
    assert same(V, eV) and same(T, eT)
    s.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_every_window_option_opens_a_new_window_and_async_steps_accumulate(built, dtype):
    dims = (13, 11, 10)
    A, _ = geometries(dims)
    types = np.asarray(A.type)
    s = capi.Solver(A, capi.fluid_params(dtype, *PARAMS), dtype)
    s.set_option(capi.OPT_TIME_STATS, 2)
    s.set_option(capi.OPT_TIME_STATS_GRAD, 1)
    rng = np.random.default_rng(42)
    seed = 60
    for opt, value, mode in ((capi.OPT_TIME_STATS, 1, 1), (capi.OPT_TIME_STATS_CROSS, 1, 1), (capi.OPT_TIME_STATS_EVERY, 1, 1),
                             (capi.OPT_TIME_STATS_GRAD, 1, 1)):
        do_step(s, "swap", rng, A, seed)                           # a step of the window that the option closes
        s.set_option(opt, value)
        twin = TS.TimeStats(dims, mode, gradients=True, spacing=GENERAL)
        for k in range(2):
            if k:
                s.upload_layer(capi.LAYER_CUR, near_one(rng, dims, s.dtype, A))
                s.time_step_async(DT, 1, 1)
                s.synchronize()
                cur = s.download_layer(capi.LAYER_CUR)
            else:
                cur = do_step(s, "swap", rng, A, seed + 1)
            twin.add(cur, types)
        seed += 2
        check_record(s, twin, types, "after option %d" % opt)
    s.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_allocations_are_counted_once_and_the_option_at_zero_frees_them(built, dtype):
    dims = (13, 11, 10)
    A, _ = geometries(dims)
    results = []
    for grad in (0, 1):
        s = capi.Solver(A, capi.fluid_params(dtype, *PARAMS), dtype)
        count = lambda: s.geometry_info()["device_allocs_and_frees"]      # noqa: E731
        a0 = count()
        s.set_option(capi.OPT_TIME_STATS, 1)
        s.set_option(capi.OPT_TIME_STATS_GRAD, grad)
        assert count() == a0, "nothing is allocated before a step needs it"
        seen = []
        for _ in range(3):
            s.UpdateBoundaries()
            s.TimeStep(DT, 2, 1, True)
            seen.append(count() - a0)
        assert seen == [2 + 2 * grad] * 3, "the counts and the sums of the fields; +2 once with the gradient sums"
        results.append(s.download_layer(capi.LAYER_CUR) + s.download_layer(capi.LAYER_NEXT))
        if grad:
            s.set_option(capi.OPT_TIME_STATS_GRAD, 0)              # frees the two buffers
            assert count() - a0 == 6
            s.UpdateBoundaries()
            s.TimeStep(DT, 2, 1, True)
            assert count() - a0 == 6
            s.set_option(capi.OPT_TIME_STATS_GRAD, 1)
            s.UpdateBoundaries()
            s.TimeStep(DT, 2, 1, True)
            assert count() - a0 == 8
            s.set_option(capi.OPT_TIME_STATS, 0)                   # frees all four
            assert count() - a0 == 12
        s.close()
    for a, b in zip(*results):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), "the steps compute what they compute without the option"


@pytest.mark.parametrize("dtype", DTYPES)
def test_refusals(built, dtype):
    dims = (13, 11, 10)
    A, _ = geometries(dims)
    types = np.asarray(A.type)
    params = capi.fluid_params(dtype, *PARAMS)
    s = capi.Solver(A, params, dtype)
    lib = s.lib
    for bad in (-1, 2, 9):
        assert lib.fs3d_set_option(s.h, capi.OPT_TIME_STATS_GRAD, bad) == capi.ERR_INVALID
    V, T = nan_arrays(COARSE, dtype)
    pV, pT = V.ctypes.data_as(C.c_void_p), T.ctypes.data_as(C.c_void_p)
    rows = (C.c_int * 2)(-1, -1)

    def refused(why):
        before = s.download_layer(capi.LAYER_NEXT)
        assert lib.fs3d_get_layer(s.h, pV, pT, *COARSE) == capi.ERR_INVALID, why
        assert lib.fs3d_get_layer_rows(s.h, pV, pT, *COARSE, rows) == capi.ERR_INVALID, why
        assert lib.fs3d_get_layer_dev(s.h, pV, pT, *COARSE, rows) == capi.ERR_INVALID, why      # refused before the pointers are used
        assert np.isnan(V).all() and np.isnan(T).all() and list(rows) == [-1, -1], why
        assert all(np.array_equal(a, b) for a, b in zip(s.download_layer(capi.LAYER_NEXT), before)), "no stamp either"
    rng = np.random.default_rng(43)
    s.set_option(capi.OPT_OUTPUT_GRADIENT, 2)
    s.set_option(capi.OPT_OUTPUT_SOURCE, 1)
    refused("no statistics at all")
    s.set_option(capi.OPT_TIME_STATS, 1)
    do_step(s, "swap", rng, A, 70)
    refused("a window without the gradient sums")
    assert b"FS3D_OPT_OUTPUT_GRADIENT 2" in lib.fs3d_last_error(s.h)
    s.set_option(capi.OPT_TIME_STATS_GRAD, 1)
    refused("an empty window")
    twin = TS.TimeStats(dims, 1, gradients=True, spacing=GENERAL)
    twin.add(do_step(s, "swap", rng, A, 71), types)
    for source in (0, 2, 3):
        s.set_option(capi.OPT_OUTPUT_SOURCE, source)
        refused("source %d" % source)
    s.set_option(capi.OPT_OUTPUT_SOURCE, 1)
    s.set_option(capi.OPT_OUTPUT_VECTOR, 1)
    refused("two options claim outV")
    s.set_option(capi.OPT_OUTPUT_VECTOR, 0)
    check_record(s, twin, types, "after the refusals")              # the refused context goes on
    s.close()
    # an x-slab refuses the option; a context without it goes on as ever
    slab = capi.Solver(A, params, dtype, x_range=(0, 7))
    assert lib.fs3d_set_option(slab.h, capi.OPT_TIME_STATS_GRAD, 1) == capi.ERR_UNSUPPORTED
    assert b"x-slab" in lib.fs3d_last_error(slab.h)
    slab.set_option(capi.OPT_TIME_STATS_GRAD, 0)
    slab.close()
    # a member of a group of two: the steps are refused before any launch, no swap, the layers as they were
    grp = capi.LocalGroup.__new__(capi.LocalGroup)
    grp.lib, grp.h, grp.solvers = lib, C.c_void_p(), []
    assert lib.fs3d_local_group_create(2, C.byref(grp.h)) == capi.OK
    m = capi.Solver(A, params, dtype)
    grp.solvers.append(m)
    m.set_option(capi.OPT_TIME_STATS, 1)
    m.set_option(capi.OPT_TIME_STATS_GRAD, 1)
    m.comm_init_local(grp, 0)
    fields = general_fields(dims, dtype, 72), general_fields(dims, dtype, 73)
    m.upload_layer(capi.LAYER_CUR, fields[0])
    m.upload_layer(capi.LAYER_NEXT, fields[1])
    err = C.c_double(-1.0)
    assert lib.fs3d_time_step(m.h, DT, 1, 1, 0, C.byref(err)) == capi.ERR_UNSUPPORTED
    assert b"FS3D_OPT_TIME_STATS_GRAD" in lib.fs3d_last_error(m.h) and err.value == -1.0
    assert lib.fs3d_time_step_async(m.h, DT, 1, 1) == capi.ERR_UNSUPPORTED
    assert b"member of a group" in lib.fs3d_last_error(m.h)
    for layer, want in ((capi.LAYER_CUR, fields[0]), (capi.LAYER_NEXT, fields[1])):
        assert all(np.array_equal(a, b) for a, b in zip(m.download_layer(layer), want)), "no swap, no launch"
    m.set_option(capi.OPT_OUTPUT_SOURCE, 1)
    assert lib.fs3d_get_layer(m.h, pV, pT, *COARSE) == capi.ERR_INVALID, "no candidate was counted: the window is empty"
    grp.close()


def test_driver_writes_the_python_paths_gradient_record(built, tmp_path, monkeypatch):
    from scipy.io import netcdf_file
    from test_gpu_host_driver_stats import NSTEPS, OD, driver_case, run
    monkeypatch.setenv("FS3D_DEFAULT_KERNEL", "4")
    driver = B.build_driver()
    data, cfgf = driver_case(tmp_path)
    run(driver, data, str(tmp_path / "mean"), cfgf, ["GPU", "--time-stats", "mean"])
    out = run(driver, data, str(tmp_path / "grad"), cfgf, ["GPU", "--time-stats", "mean", "--time-gradients"])
    assert out.rstrip().splitlines()[-1] == "Time statistics: %d steps, mean, gradients in %s_stats.nc" % (NSTEPS, tmp_path / "grad")
    assert open(str(tmp_path / "grad_res.nc"), "rb").read() == open(str(tmp_path / "mean_res.nc"), "rb").read()
    nodes, cfg, dt = shape2d.load_case(data, cfgf, align=True)
    s = capi.Solver(nodes, capi.fluid_params(np.float32, cfg.Re, cfg.Pr, cfg.lam), np.float32)
    s.set_option(capi.OPT_TIME_STATS, 1)
    s.set_option(capi.OPT_TIME_STATS_GRAD, 1)
    for i in range(NSTEPS):
        s.UpdateBoundaries()
        s.TimeStep(np.float32(dt), cfg.num_global, cfg.num_local, i % 10 == 0)
        if i % cfg.out_time_steps == 0:
            s.GetLayer(OD)                                         # the driver's call: the stamp on `next`
    s.set_option(capi.OPT_OUTPUT_SOURCE, 1)
    s.set_option(capi.OPT_OUTPUT_GRADIENT, 2)
    V, T = s.GetLayer(OD)
    s.close()
    f = netcdf_file(str(tmp_path / "grad_stats.nc"), "r", mmap=False)
    g = netcdf_file(str(tmp_path / "mean_stats.nc"), "r", mmap=False)
    assert f.variables["u"].shape == (3,) + OD and g.variables["u"].shape == (2,) + OD
    fV = np.stack([np.asarray(f.variables[nm][1], np.float64) for nm in "uvw"], axis=-1)
    assert np.array_equal(fV, V.astype(np.float64)) and np.array_equal(np.asarray(f.variables["T"][1], np.float64), T)
    fluid = T != 99999.0
    assert (V[fluid][:, 2] > 0).any(), "a mean strain rate"
    for nm in "uvwT":                                              # the mean first, the fluid fraction last, as without the word
        assert np.array_equal(f.variables[nm][0], g.variables[nm][0]) and np.array_equal(f.variables[nm][2], g.variables[nm][1]), nm
    f.close()
    g.close()
