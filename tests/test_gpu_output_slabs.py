"""GPU: filtered and derived result records on x-slabs (FS3D_OPT_OUTPUT_SLABS; k_get_layer_box<.., SLAB>, k_get_layer_finish, the grouped
exchange of the sampled layer's boundary planes and type planes, one all-reduce of the straddling rows' partial sums) -- in-process
groups of 2, 3 and 4 slabs on device 0, both precisions.  The rows of all ranks together must be the record of the numpy twin on the
GLOBAL grid (cmc_fluid_solver_amd/layer_output.py): bit for bit on exact fields and for the point vorticity, within the derived bound
of test_gpu_output_filter.py on general fields.  tests/test_output_slabs_cases.py shows that slabs which exchange nothing write
another record on every one of these cases.

Every test sets option 19 first: on a library without the option each of them fails there."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import output_slabs_cases as OC  # noqa: E402
from test_gpu_output_filter import (PARAMS, _driver_case, assert_within_bound, exact_fields, general_fields, make_nodes,  # noqa: E402
                                    nan_arrays, set_mode)
from cmc_fluid_solver_amd import build as B  # noqa: E402
from cmc_fluid_solver_amd import capi, grids, shape2d  # noqa: E402
from cmc_fluid_solver_amd import layer_output as LO  # noqa: E402
from cmc_fluid_solver_amd.slab import out_rows  # noqa: E402

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]
IDS = [OC.case_id(c) for c in OC.CASES]
DT = 0.05


@pytest.fixture(scope="module", autouse=True)
def _torch_first():
    import torch
    torch.cuda.init()                    # before the library opens the device


@pytest.fixture(autouse=True)
def _exact_kernels(monkeypatch):
    """New contexts start on the bit-exact kernels: slabs and a single context then hold the same fields after the same steps."""
    monkeypatch.setenv("FS3D_DEFAULT_KERNEL", "4")


def group(nodes, nranks, dtype, next_fields=None):
    grp = capi.LocalGroup(nodes, capi.fluid_params(dtype, *PARAMS), nranks, dtype)
    for s in grp.solvers:
        s.set_option(capi.OPT_OUTPUT_SLABS, 1)
        if next_fields is not None:
            s.upload_layer(capi.LAYER_NEXT, [f[s.x0:s.x1] for f in next_fields])
    return grp


def record(grp, outdims, filter, vector, before=None):
    """One collective record: every rank writes its rows into shared NaN-filled arrays of the whole output grid"""
    s0 = grp.solvers[0]
    od = tuple(o or d for o, d in zip(outdims, s0.gdims))
    V, T = nan_arrays(od, s0.dtype.type)

    def work(rank, s):
        if before:
            before(s)
        set_mode(s, filter, vector)
        return s.GetLayerRows(V, T, outdims)
    rows = grp.run(work)
    assert rows == [out_rows(s.x0, s.x1, s0.gdims[0], od[0]) for s in grp.solvers]
    assert not np.isnan(V).any() and not np.isnan(T).any(), "every row has an owner"
    return V, T


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", OC.CASES, ids=IDS)
def test_exact_fields_equal_the_global_record_bit_for_bit(built, case, dtype):
    dims, od, nranks = case
    nodes = make_nodes(dims, OC.POW2)
    fields = exact_fields(dims, dtype, 21)
    grp = group(nodes, nranks, dtype, fields)
    for filter, vector in OC.MODES:
        V, T = record(grp, od, filter, vector)
        eV, eT = LO.layer_output(nodes.type, fields, od, filter, vector, OC.POW2)
        assert V.dtype == eV.dtype and np.array_equal(V, eV) and np.array_equal(T, eT), (filter, vector)
    grp.close()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", OC.CASES, ids=IDS)
def test_general_fields_point_vorticity_bit_for_bit_and_box_means_within_the_bound(built, case, dtype):
    dims, od, nranks = case
    nodes = make_nodes(dims, OC.GENERAL)
    fields = general_fields(dims, dtype, 22)
    grp = group(nodes, nranks, dtype, fields)
    V, T = record(grp, od, 0, 1)
    eV, eT = LO.layer_output(nodes.type, fields, od, 0, 1, OC.GENERAL)
    assert np.array_equal(V, eV) and np.array_equal(T, eT), "the curl across the cuts, general spacings"
    for vector in (0, 1):
        V, T = record(grp, od, 1, vector)
        assert_within_bound(nodes.type, fields, od, vector, OC.GENERAL, V, T, "%s %s vector %d" % (OC.case_id(case), np.dtype(dtype).name, vector))
    grp.close()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", [OC.CASES[1], OC.CASES[3]], ids=[IDS[1], IDS[3]])
def test_the_device_entry_writes_the_same_rows(built, case, dtype):
    import torch
    dims, od, nranks = case
    nodes = make_nodes(dims, OC.POW2)
    fields = exact_fields(dims, dtype, 23)
    grp = group(nodes, nranks, dtype, fields)
    td = torch.float32 if dtype == np.float32 else torch.float64
    for filter, vector in OC.MODES:
        hV, hT = record(grp, od, filter, vector)
        dV = torch.full(tuple(od) + (3,), float("nan"), dtype=td, device="cuda")
        dT = torch.full(tuple(od), float("nan"), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()

        def work(rank, s):
            rows = s.GetLayerDev(dV, dT, od)
            s.synchronize()
            return rows
        assert grp.run(work) == [out_rows(s.x0, s.x1, dims[0], od[0]) for s in grp.solvers]
        assert np.array_equal(dV.cpu().numpy(), hV) and np.array_equal(dT.cpu().numpy(), hT), (filter, vector)
    grp.close()


STAT_DIMS, STAT_OD, STAT_RANKS = (23, 13, 11), (5, 4, 7), 3
SOURCES = [(1, 0), (2, 0), (2, 1), (2, 2), (3, 0)]                   # (source, moment)


@pytest.mark.parametrize("dtype", DTYPES)
def test_time_statistics_of_every_source_through_the_filter_and_the_curl(built, dtype):
    """Four accumulated steps on a group and on a single context (the exact kernels: the same fields, so the same sums per cell).
    The single context's point record at full resolution IS the stamped statistic layer Q; the group's filtered and derived records
    are held to the twin's rule on that Q: the point vorticity bit for bit, the box means within the derived bound -- and bit for bit
    where the single context's own record is (the fluid fraction: every sum of n / N over a box is exact)."""
    nodes = grids.box_with_obstacle(*STAT_DIMS)
    spacing = (nodes.dx, nodes.dy, nodes.dz)
    base = [np.ascontiguousarray(a, dtype) for a in (nodes.vx, nodes.vy, nodes.vz, nodes.T)]
    start = grids.perturb(base, seed=8)

    def steps(rank, s):
        s.set_option(capi.OPT_TIME_STATS, 2)
        s.set_option(capi.OPT_TIME_STATS_CROSS, 1)
        s.upload_layer(capi.LAYER_CUR, [f[s.x0:s.x1] for f in start])
        for _ in range(4):
            s.UpdateBoundaries()
            s.TimeStep(DT, 2, 1, True)
    grp = group(nodes, STAT_RANKS, dtype)
    grp.run(steps)
    one = capi.Solver(nodes, capi.fluid_params(dtype, *PARAMS), dtype)
    steps(0, one)
    for source, moment in SOURCES:
        def select(s):
            s.set_option(capi.OPT_OUTPUT_SOURCE, source)
            s.set_option(capi.OPT_OUTPUT_MOMENT, moment)
        select(one)
        set_mode(one, 0, 0)
        qV, qT = one.GetLayer()
        Q = [np.ascontiguousarray(qV[..., v]) for v in range(3)] + [qT.astype(dtype)]
        assert np.array_equal(Q[3].astype(np.float64), qT)
        for filter, vector in OC.MODES:
            if vector and moment:
                continue                                       # refused on one GPU as well: the curl of a stress layer
            V, T = record(grp, STAT_OD, filter, vector, before=select)
            what = "source %d moment %d filter %d vector %d %s" % (source, moment, filter, vector, np.dtype(dtype).name)
            if filter:
                assert_within_bound(nodes.type, Q, STAT_OD, vector, spacing, V, T, what)
            else:
                eV, eT = LO.layer_output(nodes.type, Q, STAT_OD, 0, 1, spacing)
                assert np.array_equal(V, eV) and np.array_equal(T, eT), what
            if source == 3 and not vector:
                set_mode(one, filter, vector)
                sV, sT = one.GetLayer(STAT_OD)
                assert np.array_equal(V, sV) and np.array_equal(T, sT), what
    one.close()
    grp.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_records_after_every_step_leave_the_fields_of_a_run_without_records(built, dtype):
    """The record overwrites the ghost planes of `next` with the neighbours' stamped planes; every time step exchanges them again.
    K steps with a filtered curl record after each one against K steps without: the same bits in cur and next, on every cell that
    is not NODE_OUT (those carry the stamp of a record, as after every record on one GPU)."""
    nodes = grids.box_with_obstacle(*STAT_DIMS)
    base = [np.ascontiguousarray(a, dtype) for a in (nodes.vx, nodes.vy, nodes.vz, nodes.T)]
    start = grids.perturb(base, seed=9)
    K = 3

    def run(with_records):
        grp = group(nodes, 3, dtype)
        V, T = nan_arrays(STAT_OD, dtype)

        def work(rank, s):
            s.upload_layer(capi.LAYER_CUR, [f[s.x0:s.x1] for f in start])
            set_mode(s, 1, 1)
            for _ in range(K):
                s.UpdateBoundaries()
                s.TimeStep(DT, 2, 1, True)
                if with_records:
                    s.GetLayerRows(V, T, STAT_OD)
            return s.download_layer(capi.LAYER_CUR), s.download_layer(capi.LAYER_NEXT)
        res = grp.run(work)
        grp.close()
        return [np.concatenate([r[l][v] for r in res], axis=0) for l in (0, 1) for v in range(4)], V
    with_, V = run(True)
    without, _ = run(False)
    assert not np.isnan(V).any() and (V != 0).any()
    keep = nodes.type != grids.NODE_OUT
    assert (nodes.type == grids.NODE_IN).any() and any(np.abs(f[keep]).max() > 0 for f in without[:3])
    for a, b in zip(with_, without):
        assert np.array_equal(a[keep], b[keep])


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_geometry_update_is_seen_by_the_next_record(built, dtype):
    """The obstacle moves between two records; 4 slabs of 23 planes cut at 6, 12 and 18.  The second record is the twin's of the new
    types -- the type planes at the cuts are derived again from the new code table -- and not the one of the old types."""
    dims, od, nranks = (23, 13, 11), (5, 4, 7), 4
    nodes = make_nodes(dims, OC.POW2, out_block=False)
    moved = grids.box_with_obstacle(*dims, lo=0.2, hi=0.5)
    moved.dx, moved.dy, moved.dz = OC.POW2
    cuts = [c[0] for c in OC.cuts_of(dims[0], nranks)[1:]]
    assert any((nodes.type[x - 1:x + 1] != moved.type[x - 1:x + 1]).any() for x in cuts), "the types change on a plane at a cut"
    fields = exact_fields(dims, dtype, 17)
    grp = group(nodes, nranks, dtype, fields)
    record(grp, od, 1, 1)

    def update(rank, s):
        s.update_nodes_slab(moved)
        s.upload_layer(capi.LAYER_NEXT, [f[s.x0:s.x1] for f in fields])
    grp.run(update)
    for filter, vector in OC.MODES:
        V, T = record(grp, od, filter, vector)
        eV, eT = LO.layer_output(moved.type, fields, od, filter, vector, OC.POW2)
        oV, _ = LO.layer_output(nodes.type, fields, od, filter, vector, OC.POW2)
        assert np.array_equal(V, eV) and np.array_equal(T, eT) and not np.array_equal(V, oV), (filter, vector)
    grp.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_refusals(built, dtype):
    dims, od = (23, 13, 11), (5, 4, 7)
    nodes = make_nodes(dims, OC.GENERAL, out_block=False)
    fields = exact_fields(dims, dtype, 18)
    params = capi.fluid_params(dtype, *PARAMS)
    grp = group(nodes, 2, dtype, fields)
    lone = capi.Solver(nodes, params, dtype, x_range=(5, 17))
    lone.upload_layer(capi.LAYER_NEXT, [f[5:17] for f in fields])
    for bad in (-1, 2):
        assert lone.lib.fs3d_set_option(lone.h, capi.OPT_OUTPUT_SLABS, bad) == capi.ERR_INVALID
    lone.set_option(capi.OPT_OUTPUT_SLABS, 1)
    rows = (C.c_int * 2)(-1, -1)

    def untouched(s, call):
        before = s.download_layer(capi.LAYER_NEXT)
        V, T = nan_arrays(od, dtype)
        assert call(s, V.ctypes.data_as(C.c_void_p), T.ctypes.data_as(C.c_void_p)) == capi.ERR_UNSUPPORTED
        assert np.isnan(V).all() and np.isnan(T).all() and list(rows) == [-1, -1]
        assert all(np.array_equal(a, b) for a, b in zip(s.download_layer(capi.LAYER_NEXT), before)), "no stamp either"
    for filter, vector in OC.MODES:
        # a lone slab in no group: all three entries
        set_mode(lone, filter, vector)
        untouched(lone, lambda s, pV, pT: s.lib.fs3d_get_layer(s.h, pV, pT, *od))
        untouched(lone, lambda s, pV, pT: s.lib.fs3d_get_layer_rows(s.h, pV, pT, *od, rows))
        untouched(lone, lambda s, pV, pT: s.lib.fs3d_get_layer_dev(s.h, pV, pT, *od, rows))
        assert b"lone x-slab" in lone.lib.fs3d_last_error(lone.h)
        # the own-planes entry on a member of a group: refused on one rank alone, no peer is asked
        s = grp.solvers[1]
        set_mode(s, filter, vector)
        untouched(s, lambda s, pV, pT: s.lib.fs3d_get_layer(s.h, pV, pT, *od))
        assert b"x-slab" in s.lib.fs3d_last_error(s.h)
    # the time-statistics refusals come before any exchange: one rank alone returns, its peer never calls
    s = grp.solvers[0]
    set_mode(s, 1, 1)
    V, T = nan_arrays(od, dtype)
    pV, pT = V.ctypes.data_as(C.c_void_p), T.ctypes.data_as(C.c_void_p)
    s.set_option(capi.OPT_OUTPUT_SOURCE, 1)                    # no statistics are kept
    assert s.lib.fs3d_get_layer_rows(s.h, pV, pT, *od, rows) == capi.ERR_INVALID
    s.set_option(capi.OPT_TIME_STATS, 2)                       # an empty window
    assert s.lib.fs3d_get_layer_rows(s.h, pV, pT, *od, rows) == capi.ERR_INVALID
    s.set_option(capi.OPT_OUTPUT_SOURCE, 2)
    s.set_option(capi.OPT_OUTPUT_MOMENT, 1)                    # no cross sums
    assert s.lib.fs3d_get_layer_dev(s.h, pV, pT, *od, rows) == capi.ERR_INVALID
    assert np.isnan(V).all() and np.isnan(T).all() and list(rows) == [-1, -1]
    for opt in (capi.OPT_OUTPUT_MOMENT, capi.OPT_OUTPUT_SOURCE, capi.OPT_TIME_STATS):
        s.set_option(opt, 0)
    # ... and the group is as usable as before
    V, T = record(grp, od, 1, 1)
    eV, eT = LO.layer_output(nodes.type, fields, od, 1, 1, OC.GENERAL, exact_sum=True)
    assert np.array_equal(T, eT), "exact fields: the temperature means are the twin's"
    assert_within_bound(nodes.type, fields, od, 1, OC.GENERAL, V, T, "after the refusals")
    lone.close()
    grp.close()
    # no effect on a whole-grid context
    one = capi.Solver(nodes, params, dtype)
    one.upload_layer(capi.LAYER_NEXT, fields)
    res = []
    for on in (0, 1):
        one.set_option(capi.OPT_OUTPUT_SLABS, on)
        for filter, vector in [(0, 0)] + OC.MODES:
            set_mode(one, filter, vector)
            V, T = nan_arrays(od, dtype)
            assert one.GetLayerRows(V, T, od) == (0, od[0])
            res.append((V, T, one.GetLayer(od), one.get_layer_info()))
    for a, b in zip(res[:4], res[4:]):
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[3] == b[3]
        assert np.array_equal(a[2][0], b[2][0]) and np.array_equal(a[2][1], b[2][1])
    one.close()


def test_nothing_is_allocated_from_the_second_identical_call_on(built):
    dims, od, nranks = OC.CASES[1]
    nodes = grids.box_with_obstacle(*dims)
    grp = group(nodes, nranks, np.float32)

    def work(rank, s):
        s.set_option(capi.OPT_TIME_STATS, 1)
        for _ in range(2):
            s.UpdateBoundaries()
            s.TimeStep(DT, 1, 1, True)
        V, T = nan_arrays(od, np.float32)
        allocs = []
        for source in (0, 1):
            s.set_option(capi.OPT_OUTPUT_SOURCE, source)
            set_mode(s, 1, 1)
            for _ in range(3):
                s.GetLayerRows(V, T, od)
                allocs.append(s.get_layer_info()["device_allocs"])
        return allocs
    for rank, a in enumerate(grp.run(work)):
        print("rank", rank, "device allocations after each call", a)
        assert a[0] >= 1 and a[1] == a[2] == a[0] and a[3] > a[2] and a[4] == a[5] == a[3], (rank, a)
    grp.close()


def test_a_larger_record_counts_only_the_buffers_that_grow(built):
    """23 -> 5 on 3 slabs, rows 1 and 3 straddle, every rank owns rows.  The first filtered curl record of the time mean allocates
    four buffers per rank: staging, type planes, partial sums, statistic layer.  A record of four times the samples per row grows
    the staging buffer and the partial sums; the type planes and the statistic layer hold: two more, not four."""
    dims, od, nranks = OC.CASES[1]
    large = (od[0], 2 * od[1], 2 * od[2])
    nodes = grids.box_with_obstacle(*dims)
    grp = group(nodes, nranks, np.float32)

    def work(rank, s):
        s.set_option(capi.OPT_TIME_STATS, 1)
        s.UpdateBoundaries()
        s.TimeStep(DT, 1, 1, True)
        s.set_option(capi.OPT_OUTPUT_SOURCE, 1)
        set_mode(s, 1, 1)
        allocs = []
        for o in (od, od, large, large, od):
            V, T = nan_arrays(o, np.float32)
            s.GetLayerRows(V, T, o)
            allocs.append(s.get_layer_info()["device_allocs"])
        return allocs
    for rank, a in enumerate(grp.run(work)):
        assert a == [4, 4, 6, 6, 6], (rank, a)
    grp.close()


# ---- the driver word ---------------------------------------------------------------------------------------------------------

def bound_check(type, fields, outdims, V, T, what):
    """assert_within_bound (test_gpu_output_filter.py: the same yardstick m* = fsum / n and the same bound, velocity records) for an
    output grid of the size of the shipped configs': the cells of every box are gathered into one array per axis offset, and the two
    exact sums per sample are math.fsum over a row of it (cells outside the box or not NODE_IN enter as zeros, which change no sum)."""
    type = np.asarray(type)
    st = LO.stamp(type, fields)
    ax = [LO.boxes(g, o) for g, o in zip(type.shape, outdims)]
    w = [int((hi - lo).max()) for lo, hi in ax]
    idx, ok = [], []
    for (lo, hi), g, wa in zip(ax, type.shape, w):
        off = lo[:, None] + np.arange(wa)[None, :]
        ok.append(off < hi[:, None])
        idx.append(np.minimum(off, g - 1))
    sel = (idx[0][:, None, None, :, None, None], idx[1][None, :, None, None, :, None], idx[2][None, None, :, None, None, :])
    inbox = ok[0][:, None, None, :, None, None] & ok[1][None, :, None, None, :, None] & ok[2][None, None, :, None, None, :]
    m = (inbox & (type[sel] == grids.NODE_IN)).reshape(len(ax[0][0]), len(ax[1][0]), len(ax[2][0]), -1)
    n = m.sum(axis=-1)
    eV, eT = LO.layer_output(type, fields, outdims)
    empty = n == 0
    assert np.array_equal(V[empty], eV[empty]) and np.array_equal(T[empty], eT[empty]), what
    used = 0.0
    for c in range(4):
        q = np.where(m, st[c][sel].reshape(m.shape).astype(np.float64), 0.0)[~empty]
        nn = n[~empty].astype(np.float64)
        mstar = np.array([math.fsum(r) for r in q.tolist()]) / nn
        A = np.array([math.fsum(r) for r in np.abs(q).tolist()])
        got = (V[..., c] if c < 3 else T)[~empty].astype(np.float64)
        bound = (nn + 2) * 2.0 ** -53 * A / nn + (2.0 ** -24 * np.abs(mstar) if c < 3 else 0.0)
        err = np.abs(got - mstar)
        assert (err <= bound).all(), (what, c, float((err - bound).max()))
        if (bound > 0).any():                                  # (a component that is zero on every fluid cell has no bound to use)
            used = max(used, float((err[bound > 0] / bound[bound > 0]).max()))
    print("%s: largest error / bound = %.3f" % (what, used))


def run_driver(driver, data, prefix, cfgf, words, nsteps=11):
    subprocess.run([driver, data, prefix, cfgf, "align"] + words + ["--steps", str(nsteps)], check=True, capture_output=True, text=True, timeout=300)
    return prefix + "_res.nc"


def test_driver_slab_word_on_a_full_resolution_output_writes_the_single_gpu_bytes(built, tmp_path):
    driver = B.build_driver()
    usage = subprocess.run([driver], capture_output=True, text=True, timeout=60).stdout
    assert "[--output-filter point|box] [--slab-output-filter point|box]" in usage, "a driver without the word ignores it and samples points"
    data, cfgf = _driver_case(tmp_path, (70, 64, 66))
    one = run_driver(driver, data, str(tmp_path / "one"), cfgf, ["GPU", "--output-filter", "box"])
    two = run_driver(driver, data, str(tmp_path / "two"), cfgf, ["GPU", "2", "--same-device", "--slab-output-filter", "box"])
    a, b = open(one, "rb").read(), open(two, "rb").read()
    assert len(a) > 1000 and a == b


@pytest.mark.parametrize("nslabs", [2, 6])
def test_driver_slab_word_on_the_configs_coarse_output_stays_within_the_bound(built, tmp_path, nslabs):
    """54 rows of 64 planes, boxes of one or two planes: the cut of 2 slabs, 32, is a box edge (27 * 64 / 54) and no row straddles
    it -- as for 3, 4 and 5 slabs --; of the cuts of 6 slabs, 44 lies inside the box [43, 45) of row 37."""
    from scipy.io import netcdf_file
    driver = B.build_driver()
    data, cfgf = _driver_case(tmp_path)                        # the shipped config: 54 x 54 x 52 samples of 64^3 cells
    nsteps = 11
    res = run_driver(driver, data, str(tmp_path / "two"), cfgf, ["GPU", str(nslabs), "--same-device", "--slab-output-filter", "box"], nsteps)
    nodes, cfg, dt = shape2d.load_case(data, cfgf, align=True)
    od = (cfg.outdimx, cfg.outdimy, cfg.outdimz)
    assert all(o < d for o, d in zip(od, nodes.shape))
    assert LO.straddling_rows(OC.cuts_of(nodes.shape[0], nslabs), nodes.shape[0], od[0]) == {2: [], 6: [37]}[nslabs]
    s = capi.Solver(nodes, capi.fluid_params(np.float32, cfg.Re, cfg.Pr, cfg.lam), np.float32)
    layers = []
    for i in range(nsteps):
        s.UpdateBoundaries()
        s.TimeStep(np.float32(dt), cfg.num_global, cfg.num_local, i % 10 == 0)
        if i % cfg.out_time_steps == 0:
            s.GetLayer(od)                                     # the driver's call: the stamp
            layers.append(s.download_layer(capi.LAYER_NEXT))
    s.close()
    f = netcdf_file(res, "r", mmap=False)
    assert f.variables["u"].shape == (len(layers),) + od and len(layers) == 2
    point_differs = False
    for r, fields in enumerate(layers):
        V = np.stack([np.asarray(f.variables[nm][r], np.float64) for nm in "uvw"], axis=-1)
        T = np.ascontiguousarray(f.variables["T"][r], np.float64)
        assert np.array_equal(V, V.astype(np.float32)), "the file holds the library's fp32 samples"
        bound_check(nodes.type, fields, od, V.astype(np.float32), T, "driver record %d on %d slabs" % (r, nslabs))
        point_differs = point_differs or not np.array_equal(V.astype(np.float32), LO.layer_output(nodes.type, fields, od)[0])
    f.close()
    assert point_differs, "the box mean is not the point sample on this output grid"
