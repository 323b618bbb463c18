"""GPU: the wall loads as a result record (FS3D_OPT_OUTPUT_WALL 1 and 2: the modes 3 and 4 of SlabCells::vec_of and the carrier test of
k_get_layer_box, csrc/kernels_output.hip), as a time statistic (FS3D_OPT_TIME_STATS_WALL: k_time_wall, csrc/kernels_stats.hip) and its
read-out (FS3D_OPT_OUTPUT_WALL 3 and 4: k_time_wall_layer) against the numpy twins, layer_output.wall_loads and
time_stats.TimeStats(wall=True).

As in test_gpu_time_stats_gradients.py the twin is fed the layers downloaded from the same context, so the rounding of the sweeps
plays no part, and the step kinds are that file's: `real`, `fresh` and `swap` (general fields over 1e-3 .. 1e3 uploaded into `next`,
wall cells included, so F[B] != 0).  The loads are the twin's bit for bit: the full-resolution record and the gather are array_equal.
Through filter 1 the bound is the one derived in test_gpu_output_filter.py, with C the carriers (values 1, 2) or the cells with
nw >= 1 that are not NODE_OUT now (values 3, 4): for a box of n members whose |q| sum to A, the double sum of the kernel, in any
order, is within (n - 1) u A of the exact one (u = 2^-53), the division adds one rounding and outV one rounding to R, so
|got - m*| <= (n + 2) u A / n + eps_R |m*| with m* the exact mean (math.fsum) -- derived, not measured.
Every test sets option 22 or 23 first: on a library without them each of them fails there."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import open_run_cases as OC  # noqa: E402
from test_gpu_output_filter import general_fields, nan_arrays  # noqa: E402
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
NOSLIP = grids.BC_NOSLIP
# name -> (dims, plan): one fluid cell and six carriers; the shared START/END cell of a one-cell plate; dimz % 4 != 0, corners with
# two and three faces, carriers that come and go, real steps; z faces across a wave edge and across a chunk edge, on both sides;
# open fluid runs in X, Y and Z and an IN-typed first cell of Z lines
CASES = {"one_cell": ((3, 3, 3), ("swap",) * 3), "plate": ((7, 5, 6), ("swap",) * 3),
         "obstacle": ((13, 11, 10), ("real", "swap", "fresh", "real", "swap")), "wave_edge": ((9, 7, 70), ("swap",) * 4),
         "chunk_edge": ((4, 3, 261), ("swap",) * 4), "open_run": ((28, 24, 32), ("swap",) * 3)}
RUNS = [(name, 1) for name in CASES] + [("obstacle", 2), ("wave_edge", 2)]


@pytest.fixture(scope="module", autouse=True)
def _torch_first():
    import torch
    torch.cuda.init()                    # before the library opens the device


def wall_cell(n, cell, v=(0.25, -0.5, 0.125), T=1.5):
    grids._set_bound(n, cell, NOSLIP, NOSLIP, v, T)


def geometries(name):
    """(A, B): the geometry of the window and one that moves carriers"""
    dims = CASES[name][0]
    if name == "obstacle":
        A, Bg = grids.box_with_obstacle(*dims, lo=0.25, hi=0.55), grids.box_with_obstacle(*dims, lo=0.45, hi=0.75)
        for n in (A, Bg):                                          # a heat flux on the obstacle too (its temperature condition is FREE as built)
            inside = np.zeros(n.shape, bool)
            inside[1:-1, 1:-1, 1:-1] = True
            n.bc_temp[inside & (n.type == grids.NODE_BOUND)] = NOSLIP
    elif name == "open_run":
        g = OC.grid("all_three")
        A = grids.Nodes(*dims, g.dx, g.dy, g.dz, *[np.array(a) for a in (g.type, g.bc_vel, g.bc_temp, g.vx, g.vy, g.vz, g.T)])
        Bg = A
    else:
        A, Bg = grids.box(*dims), grids.box(*dims)
        if name == "plate":
            for n, i in ((A, 3), (Bg, 4)):
                wall_cell(n, (i, slice(1, -1), slice(1, -1)))
        elif name == "wave_edge":                                  # a wall at k = 63 faces the fluid at 64 and the other way round
            for n, ka, kb in ((A, 63, 64), (Bg, 64, 63)):
                wall_cell(n, (4, 3, ka))
                wall_cell(n, (5, 2, kb))
                wall_cell(n, (2, 4, slice(62, 66)), v=(0.0, 0.0, 1.0))       # a run of walls over the edge: x and y faces only
        elif name == "chunk_edge":
            for n, ka, kb in ((A, 255, 256), (Bg, 256, 255)):
                wall_cell(n, (1, 1, ka))
                wall_cell(n, (2, 1, kb))
    for n in (A, Bg):
        n.dx, n.dy, n.dz = GENERAL
    return A, Bg


def carriers(nodes):
    return np.logical_or.reduce(LO.exposed_faces(np.asarray(nodes.type)))


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


def assert_box_bound(members, q, outdims, V, T, what):
    """The derived bound of the module docstring, sample by sample, for the mean over `members` of the per-cell quantities q (four
    stamped arrays); a box without a member is the point sample, bit for bit.  Prints the largest share of the bound that was used."""
    eps = 2.0 ** -24 if q[0].dtype == np.float32 else 2.0 ** -53
    ax = [LO.boxes(g, o) for g, o in zip(members.shape, outdims)]
    used, boxes_with, boxes_without = 0.0, 0, 0
    for i, (x0, x1) in enumerate(zip(*ax[0])):
        for j, (y0, y1) in enumerate(zip(*ax[1])):
            for k, (z0, z1) in enumerate(zip(*ax[2])):
                box = (slice(x0, x1), slice(y0, y1), slice(z0, z1))
                m = members[box]
                n = int(m.sum())
                if n == 0:
                    boxes_without += 1
                    assert all(V[i, j, k, c] == q[c][x0, y0, z0] for c in range(3)) and T[i, j, k] == np.float64(q[3][x0, y0, z0]), (what, i, j, k)
                    continue
                boxes_with += 1
                for c in range(4):
                    vals = q[c][box][m].astype(np.float64)
                    A, mstar = math.fsum(np.abs(vals)), math.fsum(vals) / n
                    got = float(V[i, j, k, c]) if c < 3 else T[i, j, k]
                    bound = (n + 2) * 2.0 ** -53 * A / n + (eps * abs(mstar) if c < 3 else 0.0)
                    err = abs(got - mstar)
                    assert err <= bound, (what, (i, j, k), c, n, err, bound)
                    if bound > 0:
                        used = max(used, err / bound)
    print("%s: largest error / bound = %.3f (%d boxes with members, %d without)" % (what, used, boxes_with, boxes_without))
    return boxes_with, boxes_without


def check_layer_records(s, nodes, fields, what):
    """FS3D_OPT_OUTPUT_WALL 1 and 2 on the sampled layer, whose fields the caller has downloaded: array_equal at full resolution and
    through the gather, the bound through filter 1"""
    nu, kappa = s.params[1], s.params[2]
    for value, mode in ((1, LO.WALL_VECTOR), (2, LO.WALL_SCALARS)):
        s.set_option(capi.OPT_OUTPUT_WALL, value)
        for outdims in ((0, 0, 0), COARSE):
            V, T = s.GetLayer(outdims)
            eV, eT = LO.layer_output(nodes, fields, outdims, LO.POINT, mode, GENERAL, nu=nu, kappa=kappa)
            assert same(V, eV) and same(T, eT), (what, value, outdims)
        s.set_option(capi.OPT_OUTPUT_FILTER, 1)
        V, T = s.GetLayer(COARSE)
        q = LO.cell_quantities(nodes, fields, mode, GENERAL, nu, kappa)
        assert_box_bound(carriers(nodes), q, COARSE, V, T, "%s value %d box mean" % (what, value))
        # (the twin's exact_sum record is the same yardstick: m* rounded once)
        eV, eT = LO.layer_output(nodes, fields, COARSE, LO.BOX, mode, GENERAL, exact_sum=True, nu=nu, kappa=kappa)
        assert eV.shape == V.shape and eT.shape == T.shape
        V0, T0 = s.GetLayer((0, 0, 0))                             # every box one cell: filter 1 is filter 0
        eV, eT = LO.layer_output(nodes, fields, (0, 0, 0), LO.POINT, mode, GENERAL, nu=nu, kappa=kappa)
        assert same(V0, eV) and same(T0, eT), (what, value, "filter 1 at full resolution")
        s.set_option(capi.OPT_OUTPUT_FILTER, 0)
    s.set_option(capi.OPT_OUTPUT_WALL, 0)


def check_window_records(s, twin, nodes, what):
    """With source 1: values 1 and 2 on the mean layer, values 3 and 4 from the wall sums"""
    types = np.asarray(nodes.type)
    cur = s.download_layer(capi.LAYER_CUR)
    s.set_option(capi.OPT_OUTPUT_SOURCE, 1)
    check_layer_records(s, nodes, twin.layer(TS.MEAN, cur), what + " mean layer")
    members = (twin.nw >= 1) & (types != grids.NODE_OUT)
    for which in (3, 4):
        s.set_option(capi.OPT_OUTPUT_WALL, which)
        q = LO.stamp(types, twin.wall_layer(cur, which))
        for outdims in ((0, 0, 0), COARSE):
            od = tuple(o or d for o, d in zip(outdims, s.dims))
            V, T = s.GetLayer(outdims)
            eV, eT = gather(q, od)
            assert same(V, eV) and same(T, eT), (what, which, outdims)
        s.set_option(capi.OPT_OUTPUT_FILTER, 1)
        V, T = s.GetLayer(COARSE)
        assert_box_bound(members, q, COARSE, V, T, "%s value %d box mean" % (what, which))
        s.set_option(capi.OPT_OUTPUT_FILTER, 0)
    for opt in (capi.OPT_OUTPUT_WALL, capi.OPT_OUTPUT_SOURCE):
        s.set_option(opt, 0)


def make_solver(nodes, dtype):
    params = capi.fluid_params(dtype, *PARAMS)
    s = capi.Solver(nodes, params, dtype)
    s.params = params
    return s


def make_twin(dims, s, every=1):
    return TS.TimeStats(dims, 1, every=every, wall=True, spacing=GENERAL, nu=s.params[1], kappa=s.params[2])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name,every", RUNS, ids=["%s-every%d" % r for r in RUNS])
def test_records_and_sums_equal_the_twin_with_a_geometry_that_moves(built, name, every, dtype):
    dims, plan = CASES[name]
    A, Bg = geometries(name)
    cA, cB = carriers(A), carriers(Bg)
    moves = bool((cA != cB).any())
    assert cA.any() and moves == (name not in ("one_cell", "open_run")) and (not moves or (cA & ~cB).any())
    if name == "one_cell":
        assert cA.sum() == 6 and (np.asarray(A.type) == grids.NODE_IN).sum() == 1
    if name == "plate":
        faces = LO.exposed_faces(np.asarray(A.type))
        assert (faces[0] & faces[1])[3, 1:-1, 1:-1].all(), "both x faces of the shared cell"
    if name == "wave_edge":
        faces = LO.exposed_faces(np.asarray(A.type))
        assert faces[5][4, 3, 63] and faces[4][5, 2, 64] and not faces[4][2, 4, 63] and not faces[5][2, 4, 64]
    if name == "chunk_edge":
        faces = LO.exposed_faces(np.asarray(A.type))
        assert faces[5][1, 1, 255] and faces[4][2, 1, 256]
    s = make_solver(A, dtype)
    s.set_option(capi.OPT_TIME_STATS, 1)
    s.set_option(capi.OPT_TIME_STATS_EVERY, every)
    s.set_option(capi.OPT_TIME_STATS_WALL, 1)
    twin = make_twin(dims, s, every)
    rng = np.random.default_rng(41)
    for k, kind in enumerate(plan):
        nodes = Bg if k in (1, 2) else A                            # A, B, B, A, ..: carriers go and come back
        if moves and k in (1, 3):
            s.update_nodes(nodes)
        twin.add(do_step(s, kind, rng, nodes, 50 + k), nodes)
    assert twin.N == (len(plan) + every - 1) // every and twin.nw.max() == twin.N
    if moves and every == 1:
        assert (twin.nw[twin.nw > 0] < twin.N).any(), "carriers on some steps only"
    if every == 1:                                                 # the record of `next`: general fields, wall cells included
        fields = general_fields(dims, s.dtype.type, 90)
        s.upload_layer(capi.LAYER_NEXT, fields)
        check_layer_records(s, nodes, s.download_layer(capi.LAYER_NEXT), name)
    check_window_records(s, twin, nodes, "%s every %d" % (name, every))
    # the record of the fields is what it is without the options
    s.set_option(capi.OPT_OUTPUT_SOURCE, 1)
    V, T = s.GetLayer(COARSE)
    eV, eT = gather(LO.stamp(np.asarray(nodes.type), twin.layer(1, s.download_layer(capi.LAYER_CUR))), COARSE)
    assert same(V, eV) and same(T, eT)
    s.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_options_at_zero_change_nothing_and_allocations_are_steady(built, dtype):
    A, _ = geometries("obstacle")
    results = []
    for wall in (None, 0, 1):
        s = make_solver(A, dtype)
        count = lambda: s.geometry_info()["device_allocs_and_frees"]      # noqa: E731
        a0 = count()
        s.set_option(capi.OPT_TIME_STATS, 1)
        if wall is not None:
            s.set_option(capi.OPT_TIME_STATS_WALL, wall)
            s.set_option(capi.OPT_OUTPUT_WALL, 0)
        assert count() == a0, "nothing is allocated before a step needs it"
        seen = []
        for _ in range(3):
            s.UpdateBoundaries()
            s.TimeStep(DT, 2, 1, True)
            seen.append(count() - a0)
        assert seen == [2 + 2 * bool(wall)] * 3, "the counts and the sums of the fields; +2 once with the wall sums"
        rec = list(s.GetLayer(COARSE))
        s.set_option(capi.OPT_OUTPUT_SOURCE, 1)
        rec += list(s.GetLayer(COARSE))
        s.set_option(capi.OPT_OUTPUT_SOURCE, 0)
        # with the sums on, the steps and the records of the fields are the same; the allocation count differs by the two buffers
        results.append(s.download_layer(capi.LAYER_CUR) + s.download_layer(capi.LAYER_NEXT) + rec + [np.array([seen[0] - 2 * bool(wall)])])
        if wall:
            allocs = None
            for _ in range(3):                                     # further windows and read-outs: nothing more is allocated
                s.set_option(capi.OPT_TIME_STATS_WALL, 1)
                s.UpdateBoundaries()
                s.TimeStep(DT, 2, 1, True)
                s.set_option(capi.OPT_OUTPUT_SOURCE, 1)
                s.set_option(capi.OPT_OUTPUT_WALL, 4)
                s.GetLayer(COARSE)
                s.set_option(capi.OPT_OUTPUT_WALL, 0)
                s.set_option(capi.OPT_OUTPUT_SOURCE, 0)
                assert count() - a0 == 4
                allocs = allocs if allocs is not None else s.get_layer_info()["device_allocs"]
                assert s.get_layer_info()["device_allocs"] == allocs
            s.set_option(capi.OPT_TIME_STATS_WALL, 0)              # frees the two buffers
            assert count() - a0 == 6
            s.UpdateBoundaries()
            s.TimeStep(DT, 2, 1, True)
            assert count() - a0 == 6
            s.set_option(capi.OPT_TIME_STATS_WALL, 1)
            s.UpdateBoundaries()
            s.TimeStep(DT, 2, 1, True)
            assert count() - a0 == 8
            s.set_option(capi.OPT_TIME_STATS, 0)                   # frees all four
            assert count() - a0 == 12
        s.close()
    for other in results[1:]:
        for a, b in zip(results[0], other):
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), "steps, records and windows are what they are without the options"


@pytest.mark.parametrize("dtype", DTYPES)
def test_refusals(built, dtype):
    dims = CASES["obstacle"][0]
    A, _ = geometries("obstacle")
    s = make_solver(A, dtype)
    params, lib = s.params, s.lib
    s.upload_layer(capi.LAYER_NEXT, general_fields(dims, dtype, 80))
    before_V, before_T = s.GetLayer(COARSE)
    for opt, bads in ((capi.OPT_OUTPUT_WALL, (-1, 5, 22)), (capi.OPT_TIME_STATS_WALL, (-1, 2, 9))):
        s.set_option(opt, 1)
        for bad in bads:
            assert lib.fs3d_set_option(s.h, opt, bad) == capi.ERR_INVALID
        s.set_option(opt, 1 if opt == capi.OPT_OUTPUT_WALL else 0)
    wV, wT = s.GetLayer(COARSE)                                    # the option stayed as it was: the wall record
    eV, eT = LO.layer_output(A, s.download_layer(capi.LAYER_NEXT), COARSE, LO.POINT, LO.WALL_VECTOR, GENERAL, nu=params[1], kappa=params[2])
    assert same(wV, eV) and same(wT, eT)
    V, T = nan_arrays(COARSE, dtype)
    pV, pT = V.ctypes.data_as(C.c_void_p), T.ctypes.data_as(C.c_void_p)
    rows = (C.c_int * 2)(-1, -1)

    def refused(ctx, status, why):
        before = ctx.download_layer(capi.LAYER_NEXT)
        assert lib.fs3d_get_layer(ctx.h, pV, pT, *COARSE) == status, why
        assert lib.fs3d_get_layer_rows(ctx.h, pV, pT, *COARSE, rows) == status, why
        assert lib.fs3d_get_layer_dev(ctx.h, pV, pT, *COARSE, rows) == status, why      # refused before the pointers are used
        assert np.isnan(V).all() and np.isnan(T).all() and list(rows) == [-1, -1], why
        assert all(np.array_equal(a, b) for a, b in zip(ctx.download_layer(capi.LAYER_NEXT), before)), "no stamp either"

    def default_record_stands():
        s.set_option(capi.OPT_OUTPUT_WALL, 0)
        V1, T1 = s.GetLayer(COARSE)
        assert same(V1, before_V) and same(T1, before_T)

    # two options claim outV, in either order
    for first in (True, False):
        for opt, value in ((capi.OPT_OUTPUT_VECTOR, 1), (capi.OPT_OUTPUT_GRADIENT, 1), (capi.OPT_OUTPUT_GRADIENT, 2)):
            s.set_option(capi.OPT_OUTPUT_WALL, 0)
            if first:
                s.set_option(capi.OPT_OUTPUT_WALL, 2)
                s.set_option(opt, value)
            else:
                s.set_option(opt, value)
                s.set_option(capi.OPT_OUTPUT_WALL, 2)
            refused(s, capi.ERR_INVALID, "wall with option %d = %d" % (opt, value))
            assert b"two options claim outV" in lib.fs3d_last_error(s.h)
            s.set_option(opt, 0)
    default_record_stands()
    # the time means need source 1 and a window with the wall sums and a step
    rng = np.random.default_rng(43)
    for which in (3, 4):
        s.set_option(capi.OPT_OUTPUT_WALL, which)
        refused(s, capi.ERR_INVALID, "source 0")
        s.set_option(capi.OPT_OUTPUT_SOURCE, 1)
        refused(s, capi.ERR_INVALID, "no statistics at all")
        s.set_option(capi.OPT_OUTPUT_SOURCE, 0)
    s.set_option(capi.OPT_OUTPUT_WALL, 3)
    s.set_option(capi.OPT_OUTPUT_SOURCE, 1)
    s.set_option(capi.OPT_TIME_STATS, 2)
    do_step(s, "swap", rng, A, 70)
    refused(s, capi.ERR_INVALID, "a window without the wall sums")
    assert b"FS3D_OPT_OUTPUT_WALL 3" in lib.fs3d_last_error(s.h)
    s.set_option(capi.OPT_TIME_STATS_WALL, 1)
    refused(s, capi.ERR_INVALID, "an empty window")
    twin = make_twin(dims, s)
    twin.add(do_step(s, "swap", rng, A, 71), A)
    for value in (1, 2, 3, 4):
        s.set_option(capi.OPT_OUTPUT_WALL, value)
        for source in (2, 3):
            s.set_option(capi.OPT_OUTPUT_SOURCE, source)
            refused(s, capi.ERR_INVALID, "value %d with source %d" % (value, source))
    s.set_option(capi.OPT_OUTPUT_SOURCE, 0)
    s.upload_layer(capi.LAYER_NEXT, general_fields(dims, dtype, 80))      # (the swap steps moved the layers)
    default_record_stands()
    check_window_records(s, twin, A, "after the refusals")          # the refused context goes on
    s.close()
    # an x-slab refuses both options, also with FS3D_OPT_OUTPUT_SLABS at 1; without them it goes on as ever
    slab = capi.Solver(A, params, dtype, x_range=(0, 7))
    assert lib.fs3d_set_option(slab.h, capi.OPT_TIME_STATS_WALL, 1) == capi.ERR_UNSUPPORTED
    assert b"x-slab" in lib.fs3d_last_error(slab.h)
    slab.set_option(capi.OPT_TIME_STATS_WALL, 0)
    for slabs in (0, 1):
        slab.set_option(capi.OPT_OUTPUT_SLABS, slabs)
        for value in (1, 2, 3, 4):
            slab.set_option(capi.OPT_OUTPUT_WALL, value)
            refused(slab, capi.ERR_UNSUPPORTED, "an x-slab, value %d, slabs %d" % (value, slabs))
    slab.set_option(capi.OPT_OUTPUT_WALL, 0)
    slab.set_option(capi.OPT_OUTPUT_SLABS, 0)
    slab.GetLayer(COARSE)
    slab.close()
    # a member of a group of two: the records and the steps are refused before any launch, no swap, the layers as they were
    grp = capi.LocalGroup.__new__(capi.LocalGroup)
    grp.lib, grp.h, grp.solvers = lib, C.c_void_p(), []
    assert lib.fs3d_local_group_create(2, C.byref(grp.h)) == capi.OK
    m = capi.Solver(A, params, dtype)
    grp.solvers.append(m)
    m.set_option(capi.OPT_TIME_STATS, 1)
    m.set_option(capi.OPT_TIME_STATS_WALL, 1)
    m.comm_init_local(grp, 0)
    fields = general_fields(dims, dtype, 72), general_fields(dims, dtype, 73)
    m.upload_layer(capi.LAYER_CUR, fields[0])
    m.upload_layer(capi.LAYER_NEXT, fields[1])
    err = C.c_double(-1.0)
    assert lib.fs3d_time_step(m.h, DT, 1, 1, 0, C.byref(err)) == capi.ERR_UNSUPPORTED
    assert b"FS3D_OPT_TIME_STATS_WALL" in lib.fs3d_last_error(m.h) and err.value == -1.0
    assert lib.fs3d_time_step_async(m.h, DT, 1, 1) == capi.ERR_UNSUPPORTED
    assert b"member of a group" in lib.fs3d_last_error(m.h)
    for layer, want in ((capi.LAYER_CUR, fields[0]), (capi.LAYER_NEXT, fields[1])):
        assert all(np.array_equal(a, b) for a, b in zip(m.download_layer(layer), want)), "no swap, no launch"
    for slabs in (0, 1):
        m.set_option(capi.OPT_OUTPUT_SLABS, slabs)
        m.set_option(capi.OPT_OUTPUT_WALL, 1)
        refused(m, capi.ERR_UNSUPPORTED, "a member of a group, slabs %d" % slabs)
    m.set_option(capi.OPT_OUTPUT_WALL, 0)
    m.set_option(capi.OPT_OUTPUT_SOURCE, 1)
    assert lib.fs3d_get_layer(m.h, pV, pT, *COARSE) == capi.ERR_INVALID, "no candidate was counted: the window is empty"
    grp.close()


def test_driver_writes_the_python_paths_wall_records(built, tmp_path, monkeypatch):
    from scipy.io import netcdf_file
    from test_gpu_host_driver_stats import NSTEPS, OD, driver_case, run
    monkeypatch.setenv("FS3D_DEFAULT_KERNEL", "4")
    driver = B.build_driver()
    data, cfgf = driver_case(tmp_path)
    run(driver, data, str(tmp_path / "mean"), cfgf, ["GPU", "--time-stats", "mean"])
    out = run(driver, data, str(tmp_path / "wall"), cfgf, ["GPU", "--time-stats", "mean", "--time-wall"])
    assert out.rstrip().splitlines()[-1] == "Time statistics: %d steps, mean, wall in %s_stats.nc" % (NSTEPS, tmp_path / "wall")
    assert open(str(tmp_path / "wall_res.nc"), "rb").read() == open(str(tmp_path / "mean_res.nc"), "rb").read()
    nodes, cfg, dt = shape2d.load_case(data, cfgf, align=True)
    params = capi.fluid_params(np.float32, cfg.Re, cfg.Pr, cfg.lam)
    s = capi.Solver(nodes, params, np.float32)
    s.set_option(capi.OPT_TIME_STATS, 1)
    s.set_option(capi.OPT_TIME_STATS_WALL, 1)
    twin = TS.TimeStats(nodes.shape, 1, wall=True, spacing=(nodes.dx, nodes.dy, nodes.dz), nu=params[1], kappa=params[2])
    for i in range(NSTEPS):
        s.UpdateBoundaries()
        s.TimeStep(np.float32(dt), cfg.num_global, cfg.num_local, i % 10 == 0)
        twin.add(s.download_layer(capi.LAYER_CUR), nodes)
        if i % cfg.out_time_steps == 0:
            s.GetLayer(OD)                                         # the driver's call: the stamp on `next`
    cur = s.download_layer(capi.LAYER_CUR)
    s.close()
    f = netcdf_file(str(tmp_path / "wall_stats.nc"), "r", mmap=False)
    g = netcdf_file(str(tmp_path / "mean_stats.nc"), "r", mmap=False)
    assert f.variables["u"].shape == (4,) + OD and g.variables["u"].shape == (2,) + OD
    for rec, which in ((1, 3), (2, 4)):
        V, T = gather(LO.stamp(np.asarray(nodes.type), twin.wall_layer(cur, which)), OD)
        fV = np.stack([np.asarray(f.variables[nm][rec], np.float64) for nm in "uvw"], axis=-1)
        assert np.array_equal(fV, V.astype(np.float64)) and np.array_equal(np.asarray(f.variables["T"][rec], np.float64), T), which
    assert twin.nw.max() == NSTEPS and any(q.any() for q in twin.wall_layer(cur, 4)[:1]), "a mean wall shear stress somewhere"
    for nm in "uvwT":                                              # the mean first, the fluid fraction last, as without the word
        assert np.array_equal(f.variables[nm][0], g.variables[nm][0]) and np.array_equal(f.variables[nm][3], g.variables[nm][1]), nm
    f.close()
    g.close()
