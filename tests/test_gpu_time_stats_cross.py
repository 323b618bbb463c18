"""Cross sums, moment layers and the stride of the time statistics on the device (csrc/kernels_stats.hip:
FS3D_OPT_TIME_STATS_CROSS, FS3D_OPT_OUTPUT_MOMENT, FS3D_OPT_TIME_STATS_EVERY) against their numpy twin
(cmc_fluid_solver_amd/time_stats.py).

As in test_gpu_time_stats.py, whose step plan (real, wild and fresh steps), gather and helpers serve here: every comparison is
array_equal with NaN equal to NaN, and the twin is fed the `cur` downloaded after each step of the same context.  A layer is named
by (source, moment): (1, 0) mean, (2, 0) variance, (2, 1) Reynolds stresses and k, (2, 2) heat fluxes and var_T, (3, 0) fraction."""
import ctypes as C

import numpy as np
import pytest

from cmc_fluid_solver_amd import capi, grids
from cmc_fluid_solver_amd import layer_output as LO
from cmc_fluid_solver_amd import time_stats as TS
from cmc_fluid_solver_amd.slab import out_rows, slab_range

import test_gpu_time_stats as G  # noqa: E402
from test_gpu_time_stats import COARSE, DT, DTYPES, PARAMS, PLAN, SLAB_DIMS, DeviceArray, do_step, gather, nan_arrays, obstacle, same  # noqa: E402

pytestmark = pytest.mark.gpu

ALL = ((1, 0), (2, 0), (2, 1), (2, 2), (3, 0))
OLD = ((1, 0), (2, 0), (3, 0))


def expected(twin, layer, cur, types, od):
    return gather(LO.stamp(types, twin.layer(layer[0], cur, layer[1])), od)


def select(s, layer):
    s.set_option(capi.OPT_OUTPUT_SOURCE, layer[0])
    s.set_option(capi.OPT_OUTPUT_MOMENT, layer[1])


def unselect(s):
    s.set_option(capi.OPT_OUTPUT_SOURCE, 0)
    s.set_option(capi.OPT_OUTPUT_MOMENT, 0)


def check_layers(s, twin, types, layers=ALL, outdims=((0, 0, 0), COARSE), what=""):
    cur = s.download_layer(capi.LAYER_CUR)
    for layer in layers:
        select(s, layer)
        for outdims_ in outdims:
            od = tuple(o or d for o, d in zip(outdims_, s.dims))
            eV, eT = expected(twin, layer, cur, types, od)
            V, T = s.GetLayer(outdims_)
            assert same(V, eV) and same(T, eT), (what, layer, outdims_)
    unselect(s)


def records(s, layers, outdims=COARSE):
    out = []
    for layer in layers:
        select(s, layer)
        out.append(s.GetLayer(outdims))
    unselect(s)
    return out


def allocs(s):
    return s.geometry_info()["device_allocs_and_frees"]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("dims", [(16, 12, 8), (9, 7, 5), (4, 7, 5), (40, 36, 32)])
def test_moments_equal_the_twin_on_every_launch_form(built, dims, dtype):
    """16 x 12 x 8: the vector form; 9 x 7 x 5: an odd cell count, cell by cell; 4 x 7 x 5: a multiple of 4 whose fields sit off the
    16 bytes, cell by cell too; 40 x 36 x 32: 45 workgroups"""
    nodes = obstacle(dims) if dims[2] != 5 else grids.box(*dims)
    types = np.asarray(nodes.type)
    assert (types == grids.NODE_IN).any() and (types == grids.NODE_BOUND).any()
    s = capi.Solver(nodes, capi.fluid_params(dtype, *PARAMS), dtype)
    s.set_option(capi.OPT_TIME_STATS, 2)
    s.set_option(capi.OPT_TIME_STATS_CROSS, 1)
    twin = TS.TimeStats(dims, 2, cross=True)
    rng = np.random.default_rng(21)
    for kind in PLAN:
        twin.add(do_step(s, kind, rng, nodes), types)
    before = s.download_layer(capi.LAYER_CUR), s.download_layer(capi.LAYER_NEXT)
    check_layers(s, twin, types, what=dims)
    after = s.download_layer(capi.LAYER_CUR), s.download_layer(capi.LAYER_NEXT)
    for a, b in zip(before[0] + before[1], after[0] + after[1]):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    # the moment is read for source 2 only, and the usual counts are reported
    s.set_option(capi.OPT_OUTPUT_MOMENT, 2)
    s.set_option(capi.OPT_OUTPUT_SOURCE, 1)
    V, T = nan_arrays(COARSE, dtype)
    assert s.GetLayerRows(V, T, COARSE) == (0, COARSE[0])
    info = s.get_layer_info()
    assert info["samples"] == 210 and info["bytes_to_host"] == 210 * (3 * np.dtype(dtype).itemsize + 8)
    eV, eT = expected(twin, (1, 0), after[0], types, COARSE)
    assert same(V, eV) and same(T, eT)
    # a covariance is negative somewhere: nothing clamped it
    select(s, (2, 1))
    V, T = s.GetLayer()
    assert (V[np.isfinite(V) & (V != 99999.0)] < 0).any()
    s.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_defaults_are_mode_2_as_it_was_and_the_cross_buffer_is_counted(built, dtype):
    dims = (16, 12, 8)
    nodes = obstacle(dims)
    types = np.asarray(nodes.type)
    got = {}
    for cross in (0, 1):
        s = capi.Solver(nodes, capi.fluid_params(dtype, *PARAMS), dtype)
        a0 = allocs(s)
        s.set_option(capi.OPT_TIME_STATS, 2)
        s.set_option(capi.OPT_TIME_STATS_CROSS, cross)
        s.set_option(capi.OPT_OUTPUT_MOMENT, 0)
        s.set_option(capi.OPT_TIME_STATS_EVERY, 1)
        assert allocs(s) == a0, "no option allocates"
        twin = TS.TimeStats(dims, 2)                          # the rule as it stood
        rng = np.random.default_rng(22)
        for kind in PLAN:
            twin.add(do_step(s, kind, rng, nodes), types)
        assert allocs(s) - a0 == 3 + cross
        G.check_sources(s, twin, types, (1, 2, 3), what="cross %d" % cross)
        got[cross] = records(s, OLD, (0, 0, 0)) + [s.download_layer(capi.LAYER_CUR), s.download_layer(capi.LAYER_NEXT)]
        if cross:
            # CROSS to 0 alone: one buffer goes, and the window is new
            s.set_option(capi.OPT_TIME_STATS_CROSS, 0)
            assert allocs(s) - a0 == 5
            twin = TS.TimeStats(dims, 2)
            twin.add(do_step(s, "real", rng, nodes), types)
            assert allocs(s) - a0 == 5
            G.check_sources(s, twin, types, (1, 2, 3), outdims=(COARSE,), what="after CROSS 0")
            s.set_option(capi.OPT_TIME_STATS_CROSS, 1)
            twin = TS.TimeStats(dims, 2, cross=True)
            twin.add(do_step(s, "fresh", rng, nodes), types)
            assert allocs(s) - a0 == 6
            check_layers(s, twin, types, outdims=(COARSE,), what="CROSS on again")
            s.set_option(capi.OPT_TIME_STATS, 0)
            assert allocs(s) - a0 == 10
        else:
            s.set_option(capi.OPT_TIME_STATS, 0)
            assert allocs(s) - a0 == 6
        s.UpdateBoundaries()
        s.TimeStep(DT, 1, 1, True)
        assert allocs(s) - a0 == (10 if cross else 6)
        s.close()
    # the same steps with CROSS on and off: sources 1, 2 with moment 0, and 3, `cur` and `next` bit for bit
    for (aV, aT), (bV, bT) in zip(got[0][:3], got[1][:3]):
        assert same(aV, bV) and same(aT, bT)
    for a, b in zip(got[0][3] + got[0][4], got[1][3] + got[1][4]):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    # mode 2 with CROSS on from the start to the end: 4 allocations, then 8 with the frees
    s = capi.Solver(nodes, capi.fluid_params(dtype, *PARAMS), dtype)
    a0 = allocs(s)
    s.set_option(capi.OPT_TIME_STATS_CROSS, 1)                 # the mode is 0: no effect, nothing allocated
    s.UpdateBoundaries()
    s.TimeStep(DT, 1, 1, True)
    assert allocs(s) == a0
    s.set_option(capi.OPT_TIME_STATS, 1)                       # mode 1: no cross buffer either
    s.UpdateBoundaries()
    s.TimeStep(DT, 1, 1, True)
    assert allocs(s) - a0 == 2
    s.set_option(capi.OPT_TIME_STATS, 0)
    assert allocs(s) - a0 == 4
    a0 = allocs(s)
    s.set_option(capi.OPT_TIME_STATS, 2)
    for _ in range(2):
        s.UpdateBoundaries()
        s.TimeStep(DT, 1, 1, True)
    assert allocs(s) - a0 == 4
    s.set_option(capi.OPT_TIME_STATS, 0)
    assert allocs(s) - a0 == 8
    s.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_setting_cross_or_every_opens_a_new_window_and_async_steps_accumulate(built, dtype):
    dims = (16, 12, 8)
    nodes = obstacle(dims)
    types = np.asarray(nodes.type)
    s = capi.Solver(nodes, capi.fluid_params(dtype, *PARAMS), dtype)
    s.set_option(capi.OPT_TIME_STATS, 2)
    s.set_option(capi.OPT_TIME_STATS_CROSS, 1)
    rng = np.random.default_rng(23)
    for kind in PLAN[:3]:
        do_step(s, kind, rng, nodes)
    s.set_option(capi.OPT_TIME_STATS_CROSS, 1)                 # the same value: still a new window
    twin = TS.TimeStats(dims, 2, cross=True)
    for k, kind in enumerate(PLAN[3:]):
        twin.add(do_step(s, kind, rng, nodes, use_async=k != 1), types)
    assert twin.N == 3
    check_layers(s, twin, types, what="after CROSS")
    s.set_option(capi.OPT_TIME_STATS_EVERY, 1)                 # the same value: a new window again
    twin = TS.TimeStats(dims, 2, cross=True)
    twin.add(do_step(s, "real", rng, nodes, use_async=True), types)
    twin.add(do_step(s, "wild", rng, nodes), types)
    check_layers(s, twin, types, outdims=(COARSE,), what="after EVERY")
    s.set_option(capi.OPT_TIME_STATS_EVERY, 2)                 # the count of candidates starts again: the next step is taken
    twin = TS.TimeStats(dims, 2, cross=True, every=2)
    taken = [twin.add(do_step(s, kind, rng, nodes, use_async=True), types) for kind in ("fresh", "real", "real")]
    assert taken == [True, False, True]
    check_layers(s, twin, types, outdims=(COARSE,), what="every 2")
    s.close()


def test_every_third_of_seven_mixed_steps_and_a_diverged_step_is_no_candidate(built):
    """The diverging input of test_gpu_time_stats.py (grids.perturb(.., vel=50) on the 12 x 9 x 10 box) between the candidates 3
    and 4: were it a candidate, step 4 would not be taken"""
    dtype, dims = np.float32, (12, 9, 10)
    nodes = grids.box_with_obstacle(*dims, h=0.04)
    types = np.asarray(nodes.type)
    base = [np.ascontiguousarray(a, dtype) for a in (nodes.vx, nodes.vy, nodes.vz, nodes.T)]
    wild = grids.perturb(base, vel=50.0)
    s = capi.Solver(nodes, capi.fluid_params(dtype, *PARAMS), dtype)
    s.set_option(capi.OPT_SWEEP_KERNEL, capi.SWEEP_EXACT)
    s.set_option(capi.OPT_TIME_STATS, 2)
    s.set_option(capi.OPT_TIME_STATS_CROSS, 1)
    s.set_option(capi.OPT_TIME_STATS_EVERY, 3)
    twin = TS.TimeStats(dims, 2, cross=True, every=3)
    taken = []
    for step in range(7):
        if step == 3:
            sane = s.download_layer(capi.LAYER_CUR)
            s.upload_layer(capi.LAYER_CUR, wild)
            with pytest.raises(capi.Fs3dError) as ei:
                s.TimeStep(DT, 1, 1, True)
            assert ei.value.status == capi.ERR_DIVERGED
            s.upload_layer(capi.LAYER_CUR, sane)
        if step % 2:
            s.time_step_async(DT, 1, 1)
            s.synchronize()
        else:
            s.UpdateBoundaries()
            s.TimeStep(DT, 1, 1, True)
        taken.append(twin.add(s.download_layer(capi.LAYER_CUR), types))
    assert taken == [True, False, False, True, False, False, True] and twin.N == 3
    check_layers(s, twin, types, what="every 3")
    # N is 3: the fluid fraction of a cell that was fluid throughout is 3 / 3
    select(s, (3, 0))
    V, T = s.GetLayer()
    assert (T[types == grids.NODE_IN] == 1.0).all()
    s.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_moving_geometry_covariances_on_cells_fluid_in_some_steps(built, dtype):
    dims = (16, 12, 10)
    A, B = obstacle(dims, 0.25, 0.55), obstacle(dims, 0.45, 0.75)
    tA, tB = np.asarray(A.type), np.asarray(B.type)
    inA, inB = tA == grids.NODE_IN, tB == grids.NODE_IN
    assert (inA & ~inB).any() and (inB & ~inA).any() and (inA & inB).any() and (~inA & ~inB).any()
    s = capi.Solver(A, capi.fluid_params(dtype, *PARAMS), dtype)
    s.set_option(capi.OPT_TIME_STATS, 2)
    s.set_option(capi.OPT_TIME_STATS_CROSS, 1)
    twin = TS.TimeStats(dims, 2, cross=True)
    rng = np.random.default_rng(24)
    for step in range(6):
        nodes = B if step % 2 else A
        if step:
            s.update_nodes(nodes)
        if step in (2, 3):                                     # a `cur` near 1 under both geometries: covariances that are not tiny
            s.upload_layer(capi.LAYER_CUR, G.near_one(rng, dims, dtype, nodes))
        s.UpdateBoundaries()
        s.TimeStep(DT, 1, 1, False)
        twin.add(s.download_layer(capi.LAYER_CUR), np.asarray(nodes.type))
    assert np.array_equal(twin.n, 3 * inA.astype(np.uint32) + 3 * inB.astype(np.uint32))
    out_now = tB == grids.NODE_OUT
    some = (inA ^ inB) & ~out_now
    assert some.any()
    cur = s.download_layer(capi.LAYER_CUR)
    for layer in ((2, 1), (2, 2)):
        select(s, layer)
        V, T = s.GetLayer()
        eV, eT = expected(twin, layer, cur, tB, dims)
        assert same(V[some], eV[some]) and same(T[some], eT[some]), layer
        assert (V[some] != 0).any() and (T[out_now] == 99999.0).all()
    unselect(s)
    check_layers(s, twin, tB, what="moving")
    s.close()


_single = {}
SLAB_OUTDIMS = ((0, 0, 0), (4, 5, 0), (50, 5, 3))


def slab_case(dtype):
    """SLAB_DIMS, exact kernels, 4 steps from a perturbed start: the single context's records of the two covariance layers (once per
    precision), each equal to the twin's"""
    key = np.dtype(dtype).name
    if key not in _single:
        nodes = grids.box_with_obstacle(*SLAB_DIMS)
        base = [np.ascontiguousarray(a, dtype) for a in (nodes.vx, nodes.vy, nodes.vz, nodes.T)]
        start = grids.perturb(base, seed=8)
        s = capi.Solver(nodes, capi.fluid_params(dtype, *PARAMS), dtype)
        s.set_option(capi.OPT_SWEEP_KERNEL, capi.SWEEP_EXACT)
        s.set_option(capi.OPT_TIME_STATS, 2)
        s.set_option(capi.OPT_TIME_STATS_CROSS, 1)
        s.upload_layer(capi.LAYER_CUR, start)
        twin = TS.TimeStats(SLAB_DIMS, 2, cross=True)
        for _ in range(4):
            s.UpdateBoundaries()
            s.TimeStep(DT, 2, 1, True)
            twin.add(s.download_layer(capi.LAYER_CUR), nodes.type)
        cur = s.download_layer(capi.LAYER_CUR)
        res = {}
        for layer in ((2, 1), (2, 2)):
            select(s, layer)
            for outdims in SLAB_OUTDIMS:
                od = tuple(o or d for o, d in zip(outdims, SLAB_DIMS))
                V, T = nan_arrays(od, dtype)
                assert s.GetLayerRows(V, T, outdims) == (0, od[0])
                eV, eT = expected(twin, layer, cur, np.asarray(nodes.type), od)
                assert same(V, eV) and same(T, eT)
                V.flags.writeable = T.flags.writeable = False
                res[layer, outdims] = (od, V, T)
        s.close()
        _single[key] = (nodes, start, res)
    return _single[key]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nslabs", [2, 3])
def test_slabs_write_the_rows_of_the_single_contexts_moment_records(built, nslabs, dtype):
    nodes, start, single = slab_case(dtype)
    gx = SLAB_DIMS[0]
    grp = capi.LocalGroup(nodes, capi.fluid_params(dtype, *PARAMS), nslabs, dtype)
    ranges = [slab_range(gx, r, nslabs) for r in range(nslabs)]

    def steps(r, sv):
        x0, x1 = ranges[r]
        sv.set_option(capi.OPT_SWEEP_KERNEL, capi.SWEEP_EXACT)
        sv.set_option(capi.OPT_TIME_STATS, 2)
        sv.set_option(capi.OPT_TIME_STATS_CROSS, 1)
        sv.upload_layer(capi.LAYER_CUR, [f[x0:x1] for f in start])
        for _ in range(4):
            sv.UpdateBoundaries()
            sv.TimeStep(DT, 2, 1, True)
    grp.run(steps)
    for (layer, outdims), (od, sV, sT) in single.items():
        V, T = nan_arrays(od, dtype)

        def rows(r, sv):
            select(sv, layer)
            return sv.GetLayerRows(V, T, outdims)
        got = grp.run(rows)
        assert got == [out_rows(x0, x1, gx, od[0]) for x0, x1 in ranges], (layer, outdims)
        assert same(V, sV) and same(T, sT), (layer, outdims)
    # the device destination gets the same rows
    for layer in ((2, 1), (2, 2)):
        od, sV, sT = single[layer, (0, 0, 0)]
        for sv, (x0, x1) in zip(grp.solvers, ranges):
            select(sv, layer)
            dV, dT = DeviceArray(np.full(od + (3,), -7.0, dtype)), DeviceArray(np.full(od, -7.0, np.float64))
            assert sv.GetLayerDev(dV.ptr, dT.ptr) == (x0, x1)
            sv.synchronize()
            hV, hT = dV.download(), dT.download()
            assert same(hV[x0:x1], sV[x0:x1]) and same(hT[x0:x1], sT[x0:x1])
            assert (hT[:x0] == -7.0).all() and (hT[x1:] == -7.0).all() and (hV[:x0] == -7.0).all() and (hV[x1:] == -7.0).all()
            dV.free()
            dT.free()
    # the filter on a slab is refused as ever, whatever the moment
    sv = grp.solvers[0]
    select(sv, (2, 1))
    sv.set_option(capi.OPT_OUTPUT_FILTER, 1)
    V, T = nan_arrays(COARSE, dtype)
    rows_ = (C.c_int * 2)(-1, -1)
    pV, pT = V.ctypes.data_as(C.c_void_p), T.ctypes.data_as(C.c_void_p)
    assert sv.lib.fs3d_get_layer_rows(sv.h, pV, pT, *COARSE, rows_) == capi.ERR_UNSUPPORTED
    assert sv.lib.fs3d_get_layer(sv.h, pV, pT, *COARSE) == capi.ERR_UNSUPPORTED
    assert np.isnan(V).all() and np.isnan(T).all() and list(rows_) == [-1, -1]
    grp.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_box_filter_runs_on_a_stress_layer(built, dtype):
    """Four steps of integers + 0.5 below 2^13 on cells that are fluid throughout: a sum of four is an integer, a mean a multiple of
    1/4, a sum of four products a multiple of 1/4 and its quarter and the product of two means multiples of 1/16 below 2^26.  Every
    covariance and variance is a multiple of 1/16 below 2^27, k of 1/32 below 2^28, and so are their roundings to fp32: a box sum of
    a few dozen of them is exact in double in any order, and the kernel equals layer_output.py's rule bit for bit."""
    dims = (16, 12, 8)
    nodes = obstacle(dims)
    types = np.asarray(nodes.type)
    s = capi.Solver(nodes, capi.fluid_params(dtype, *PARAMS), dtype)
    s.set_option(capi.OPT_TIME_STATS, 2)
    s.set_option(capi.OPT_TIME_STATS_CROSS, 1)
    twin = TS.TimeStats(dims, 2, cross=True)
    for k in range(4):
        s.upload_layer(capi.LAYER_NEXT, G.exact_fields(dims, dtype, 30 + k))
        s.TimeStep(DT, 0, 0, False)                            # zero iterations: the swap alone
        twin.add(s.download_layer(capi.LAYER_CUR), types)
    cur = s.download_layer(capi.LAYER_CUR)
    fluid = types == grids.NODE_IN
    spacing = (nodes.dx, nodes.dy, nodes.dz)
    for moment in (1, 2):
        Q = twin.layer(2, cur, moment)
        for q in Q:
            q64 = q[fluid].astype(np.float64)
            assert (q64 * 32 == np.round(q64 * 32)).all() and np.abs(q64).max() < 2 ** 28
        assert all((q[fluid] != 0).any() for q in Q) and any((q[fluid] < 0).any() for q in Q[:3])
        select(s, (2, moment))
        point = s.GetLayer(COARSE)
        s.set_option(capi.OPT_OUTPUT_FILTER, 1)
        for outdims in (COARSE, (0, 0, 0)):
            V, T = s.GetLayer(outdims)
            eV, eT = LO.layer_output(types, Q, outdims, 1, 0, spacing)
            assert same(V, eV) and same(T, eT), (moment, outdims)
            if outdims == COARSE:
                assert not np.array_equal(V, point[0]), "the option is seen"
        s.set_option(capi.OPT_OUTPUT_FILTER, 0)
    s.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_refusals_leave_destinations_rows_and_next_as_they_were(built, dtype):
    dims = (12, 9, 10)
    nodes = grids.box_with_obstacle(*dims)
    types = np.asarray(nodes.type)
    s = capi.Solver(nodes, capi.fluid_params(dtype, *PARAMS), dtype)
    lib = s.lib
    for opt, bad in ((capi.OPT_TIME_STATS_CROSS, (-1, 2, 7)), (capi.OPT_OUTPUT_MOMENT, (-1, 3, 9)),
                     (capi.OPT_TIME_STATS_EVERY, (0, -3, 2 ** 20 + 1))):
        for v in bad:
            assert lib.fs3d_set_option(s.h, opt, v) == capi.ERR_INVALID
            assert lib.fs3d_last_error(s.h)
    s.set_option(capi.OPT_TIME_STATS_EVERY, 2 ** 20)
    s.set_option(capi.OPT_TIME_STATS_EVERY, 1)
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

    def steps(twin, n=2):
        for _ in range(n):
            s.UpdateBoundaries()
            s.TimeStep(DT, 1, 1, True)
            twin.add(s.download_layer(capi.LAYER_CUR), types)
    # mode 2, CROSS on, no step yet
    s.set_option(capi.OPT_TIME_STATS, 2)
    s.set_option(capi.OPT_TIME_STATS_CROSS, 1)
    for moment in (1, 2):
        select(s, (2, moment))
        refused("N = 0, moment %d" % moment)
    assert b"no time step" in lib.fs3d_last_error(s.h)
    # mode 2 with CROSS off
    s.set_option(capi.OPT_TIME_STATS_CROSS, 0)
    twin = TS.TimeStats(dims, 2)
    steps(twin)
    for moment in (1, 2):
        select(s, (2, moment))
        refused("CROSS off, moment %d" % moment)
    assert b"FS3D_OPT_TIME_STATS_CROSS" in lib.fs3d_last_error(s.h)
    unselect(s)
    G.check_sources(s, twin, types, (1, 2, 3), outdims=(COARSE,), what="after the refusal")
    # mode 1 with CROSS on
    s.set_option(capi.OPT_TIME_STATS, 1)
    s.set_option(capi.OPT_TIME_STATS_CROSS, 1)
    twin = TS.TimeStats(dims, 1, cross=True)
    steps(twin)
    for moment in (1, 2):
        select(s, (2, moment))
        refused("mode 1, moment %d" % moment)
    s.set_option(capi.OPT_OUTPUT_SOURCE, 1)                    # the moment is not read for source 1
    gV, gT = s.GetLayer(COARSE)
    eV, eT = expected(twin, (1, 0), s.download_layer(capi.LAYER_CUR), types, COARSE)
    assert same(gV, eV) and same(gT, eT)
    # mode 2, CROSS on, steps taken: the vector option with a moment
    s.set_option(capi.OPT_TIME_STATS, 2)
    twin = TS.TimeStats(dims, 2, cross=True)
    steps(twin)
    s.set_option(capi.OPT_OUTPUT_VECTOR, 1)
    for moment in (1, 2):
        select(s, (2, moment))
        refused("vector, moment %d" % moment)
    assert b"FS3D_OPT_OUTPUT_VECTOR" in lib.fs3d_last_error(s.h)
    select(s, (2, 0))                                          # the curl of the variance is as it was: not refused
    s.GetLayer(COARSE)
    s.set_option(capi.OPT_OUTPUT_VECTOR, 0)
    # the refused context goes on
    check_layers(s, twin, types, outdims=(COARSE,), what="after the refusals")
    steps(twin, 1)
    check_layers(s, twin, types, outdims=(COARSE,), what="one more step")
    gV, gT = s.GetLayer(COARSE)
    eV, eT = gather(s.download_layer(capi.LAYER_NEXT), COARSE)
    assert same(gV, eV) and same(gT, eT)
    s.close()
