"""GPU: the invariants of the velocity gradient as a result record (FS3D_OPT_OUTPUT_GRADIENT 1: k_get_layer_box<.., 2, ..> and
k_get_layer_finish<.., 2>, csrc/kernels_output.hip) against the rule's numpy twin, layer_output.invariants.

Per cell the kernel is held to the twin bit for bit: filter 0 is array_equal on general fields and general spacings.  Filter 1 is
array_equal on the integer fields (|x| <= 63, power-of-two spacings: every operation of the rule is exact in fp32, so are the box
sums in double, whatever their order) and inside the derived bound of test_gpu_output_filter.py on general fields -- that bound
depends only on the per-cell values being the twin's.  On in-process groups of slabs with FS3D_OPT_OUTPUT_SLABS the rows are the
single context's record.  Every test sets option 20 first: on a library without the option each of them fails there."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

from test_gpu_output_filter import (COARSE, GENERAL, PARAMS, POW2, assert_within_bound, general_fields, make_nodes,  # noqa: E402
                                    nan_arrays, outdims_of, solver_with_next)
from cmc_fluid_solver_amd import capi, grids  # noqa: E402
from cmc_fluid_solver_amd import layer_output as LO  # noqa: E402
from cmc_fluid_solver_amd import time_stats as TS  # noqa: E402
from cmc_fluid_solver_amd.slab import out_rows  # noqa: E402

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]
GRIDS = [(13, 11, 10), (9, 7, 70), (6, 5, 130), (3, 3, 3)]          # dimz % 4 != 0; more than one wave along k; more than two; one defined cell
SLAB_DIMS = (23, 13, 11)
SLAB_CUTS = {2: [(0, 12), (12, 23)], 3: [(0, 11), (11, 12), (12, 23)]}      # 3: a slab of a single plane between two cuts


@pytest.fixture(scope="module", autouse=True)
def _torch_first():
    import torch
    torch.cuda.init()                    # before the library opens the device


def nodes_of(dims, spacing):
    if dims != (3, 3, 3):
        return make_nodes(dims, spacing)
    n = grids.box(*dims)
    n.dx, n.dy, n.dz = spacing
    n.type[1, 1, 1] = grids.NODE_IN                                 # (by hand: the one cell that carries invariants)
    assert int(LO.curl_defined(n.type).sum()) == 1
    return n


def integer_fields(shape, dtype, seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(-63, 64, shape).astype(dtype) for _ in range(4)]


def set_mode(s, filter, gradient, vector=0):
    s.set_option(capi.OPT_OUTPUT_FILTER, filter)
    s.set_option(capi.OPT_OUTPUT_VECTOR, vector)
    s.set_option(capi.OPT_OUTPUT_GRADIENT, gradient)


def dims_list(dims):
    return [(0, 0, 0)] + [od for od in outdims_of(dims)[1:] if dims != (3, 3, 3) or od in ((1, 1, 1), COARSE)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("dims", GRIDS)
def test_point_invariants_equal_the_twin_on_general_fields(built, dims, dtype):
    nodes = nodes_of(dims, GENERAL)
    fields = general_fields(dims, dtype, 31)
    s = solver_with_next(nodes, dtype, fields)
    set_mode(s, 0, 1)
    ok = LO.curl_defined(nodes.type)
    for outdims in dims_list(dims):
        V, T = s.GetLayer(outdims)
        eV, eT = LO.layer_output(nodes.type, fields, outdims, LO.POINT, LO.INVARIANTS, GENERAL)
        assert V.dtype == np.dtype(dtype) and np.array_equal(V, eV) and np.array_equal(T, eT), outdims
        if outdims == (0, 0, 0):
            out_cells = nodes.type == grids.NODE_OUT
            assert (V[out_cells] == 99999).all() and (V[~ok & ~out_cells] == 0).all() and (V[ok][:, 2] > 0).all() and ok.any()
    s.close()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("dims", GRIDS)
def test_box_mean_of_the_invariants_equals_the_twin_on_integer_fields(built, dims, dtype):
    nodes = nodes_of(dims, POW2)
    fields = integer_fields(dims, dtype, 32)
    s = solver_with_next(nodes, dtype, fields)
    set_mode(s, 1, 1)
    for outdims in dims_list(dims):
        V, T = s.GetLayer(outdims)
        eV, eT = LO.layer_output(nodes.type, fields, outdims, LO.BOX, LO.INVARIANTS, POW2)
        assert np.array_equal(V, eV) and np.array_equal(T, eT), outdims
    # all three entries give the same record
    import torch
    rV, rT = nan_arrays(COARSE, dtype)
    assert s.GetLayerRows(rV, rT, COARSE) == (0, COARSE[0])
    dV = torch.full(COARSE + (3,), -7.0, dtype=torch.float32 if dtype == np.float32 else torch.float64, device="cuda")
    dT = torch.full(COARSE, -7.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    assert s.GetLayerDev(dV, dT, COARSE) == (0, COARSE[0])
    s.synchronize()
    eV, eT = LO.layer_output(nodes.type, fields, COARSE, LO.BOX, LO.INVARIANTS, POW2)
    for a, b in ((rV, rT), (dV.cpu().numpy(), dT.cpu().numpy())):
        assert np.array_equal(a, eV) and np.array_equal(b, eT)
    s.close()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("dims", GRIDS[:3])
def test_box_mean_on_general_fields_stays_within_the_derived_bound(built, dims, dtype):
    nodes = nodes_of(dims, GENERAL)
    fields = general_fields(dims, dtype, 33)
    s = solver_with_next(nodes, dtype, fields)
    set_mode(s, 1, 1)
    for outdims in ((1, 1, 1), (4, 3, 3), COARSE):
        V, T = s.GetLayer(outdims)
        assert_within_bound(nodes.type, fields, outdims, LO.INVARIANTS, GENERAL, V, T, "%s %s %s invariants" % (dims, np.dtype(dtype).name, outdims))
    s.close()


def group_of(nodes, params, cuts, dtype, next_fields):
    """capi.LocalGroup with the given planes per rank (LocalGroup itself cuts evenly)"""
    grp = capi.LocalGroup.__new__(capi.LocalGroup)
    grp.lib, grp.h, grp.solvers = capi.load(), C.c_void_p(), []
    assert grp.lib.fs3d_local_group_create(len(cuts), C.byref(grp.h)) == capi.OK
    for r, cut in enumerate(cuts):
        s = capi.Solver(nodes, params, dtype=dtype, device=0, x_range=cut)
        s.comm_init_local(grp, r)
        s.set_option(capi.OPT_OUTPUT_SLABS, 1)
        s.upload_layer(capi.LAYER_NEXT, [f[s.x0:s.x1] for f in next_fields])
        grp.solvers.append(s)
    return grp


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nslabs", [2, 3])
def test_slabs_write_the_rows_of_the_single_contexts_record(built, nslabs, dtype, monkeypatch):
    monkeypatch.setenv("FS3D_DEFAULT_KERNEL", "4")
    dims, cuts = SLAB_DIMS, SLAB_CUTS[nslabs]
    params = capi.fluid_params(dtype, *PARAMS)
    cases = [(0, general_fields(dims, dtype, 34), GENERAL), (1, integer_fields(dims, dtype, 35), POW2)]
    for filter, fields, spacing in cases:
        nodes = make_nodes(dims, spacing)
        one = solver_with_next(nodes, dtype, fields)
        set_mode(one, filter, 1)
        grp = group_of(nodes, params, cuts, dtype, fields)
        for outdims in ((0, 0, 0), (5, 4, 7), (50, 3, 4)):
            od = tuple(o or d for o, d in zip(outdims, dims))
            sV, sT = one.GetLayer(outdims)
            eV, eT = LO.layer_output(nodes.type, fields, outdims, filter, LO.INVARIANTS, spacing)
            assert np.array_equal(sV, eV) and np.array_equal(sT, eT)
            V, T = nan_arrays(od, dtype)

            def work(rank, s):
                set_mode(s, filter, 1)
                return s.GetLayerRows(V, T, outdims)
            rows = grp.run(work)
            assert rows == [out_rows(x0, x1, dims[0], od[0]) for x0, x1 in cuts]
            assert np.array_equal(V, sV) and np.array_equal(T, sT), (filter, outdims)
        grp.close()
        one.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_invariants_of_the_time_mean(built, dtype):
    """Source 1 after three steps: the record is the twin's rule applied to the twin's mean layer"""
    dims = (13, 11, 10)
    nodes = grids.box_with_obstacle(*dims, lo=0.25, hi=0.7)
    types = np.asarray(nodes.type)
    spacing = (nodes.dx, nodes.dy, nodes.dz)
    s = capi.Solver(nodes, capi.fluid_params(dtype, *PARAMS), dtype)
    s.set_option(capi.OPT_TIME_STATS, 1)
    twin = TS.TimeStats(dims, 1)
    rng = np.random.default_rng(36)
    for _ in range(3):
        base = [np.asarray(a, dtype) for a in (nodes.vx, nodes.vy, nodes.vz, nodes.T)]
        s.upload_layer(capi.LAYER_CUR, [(b + rng.uniform(-0.05, 0.05, dims)).astype(dtype) for b in base])
        s.UpdateBoundaries()
        s.TimeStep(0.1, 1, 1, False)
        twin.add(s.download_layer(capi.LAYER_CUR), types)
    Q = twin.layer(TS.MEAN, s.download_layer(capi.LAYER_CUR))
    s.set_option(capi.OPT_OUTPUT_SOURCE, 1)
    set_mode(s, 0, 1)
    for outdims in ((0, 0, 0), COARSE):
        V, T = s.GetLayer(outdims)
        eV, eT = LO.layer_output(types, Q, outdims, LO.POINT, LO.INVARIANTS, spacing)
        assert np.array_equal(V, eV, equal_nan=True) and np.array_equal(T, eT), outdims
    assert (V[..., 2] > 0).any()
    s.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_refusals_leave_destinations_and_layers_as_they_were(built, dtype):
    dims, od = SLAB_DIMS, COARSE
    nodes = make_nodes(dims, GENERAL, out_block=False)
    fields = integer_fields(dims, dtype, 37)
    params = capi.fluid_params(dtype, *PARAMS)
    rows = (C.c_int * 2)(-1, -1)

    def refused(s, status, entries=("get_layer", "rows", "dev"), text=None):
        before = s.download_layer(capi.LAYER_NEXT)
        V, T = nan_arrays(od, dtype)
        pV, pT = V.ctypes.data_as(C.c_void_p), T.ctypes.data_as(C.c_void_p)
        calls = {"get_layer": lambda: s.lib.fs3d_get_layer(s.h, pV, pT, *od), "rows": lambda: s.lib.fs3d_get_layer_rows(s.h, pV, pT, *od, rows),
                 "dev": lambda: s.lib.fs3d_get_layer_dev(s.h, pV, pT, *od, rows)}           # refused before the pointers are used
        for e in entries:
            assert calls[e]() == status, e
            if text:
                assert text in s.lib.fs3d_last_error(s.h), e
        assert np.isnan(V).all() and np.isnan(T).all() and list(rows) == [-1, -1]
        assert all(np.array_equal(a, b) for a, b in zip(s.download_layer(capi.LAYER_NEXT), before)), "no stamp either"

    one = solver_with_next(nodes, dtype, fields)
    default = one.GetLayer(od)
    for bad in (3, -1, 7):
        assert one.lib.fs3d_set_option(one.h, capi.OPT_OUTPUT_GRADIENT, bad) == capi.ERR_INVALID
    again = one.GetLayer(od)
    assert np.array_equal(default[0], again[0]) and np.array_equal(default[1], again[1]), "a refused value leaves the option as it was"
    # two options claim outV: set in either order, refused by the entries
    for order in ((capi.OPT_OUTPUT_VECTOR, capi.OPT_OUTPUT_GRADIENT), (capi.OPT_OUTPUT_GRADIENT, capi.OPT_OUTPUT_VECTOR)):
        for gradient in (1, 2):
            for opt in order:
                one.set_option(opt, gradient if opt == capi.OPT_OUTPUT_GRADIENT else 1)
            refused(one, capi.ERR_INVALID, text=b"FS3D_OPT_OUTPUT_VECTOR")
            set_mode(one, 0, 0)
    # the moments of source 2 exclude it as they exclude the curl
    one.set_option(capi.OPT_TIME_STATS, 2)
    one.set_option(capi.OPT_TIME_STATS_CROSS, 1)
    one.TimeStep(0.1, 0, 0, False)
    one.upload_layer(capi.LAYER_NEXT, fields)
    one.set_option(capi.OPT_OUTPUT_SOURCE, 2)
    for moment in (1, 2):
        one.set_option(capi.OPT_OUTPUT_MOMENT, moment)
        set_mode(one, 0, 1)
        refused(one, capi.ERR_INVALID, text=b"FS3D_OPT_OUTPUT_GRADIENT 1")
    one.set_option(capi.OPT_OUTPUT_MOMENT, 0)
    set_mode(one, 0, 1)
    one.GetLayer(od)                                                # the variances take it, as they take the curl
    one.close()
    # slabs: as FS3D_OPT_OUTPUT_VECTOR 1
    grp = capi.LocalGroup(nodes, params, 2, dtype)
    lone = capi.Solver(nodes, params, dtype, x_range=(5, 17))
    for s in grp.solvers + [lone]:
        s.upload_layer(capi.LAYER_NEXT, [f[s.x0:s.x1] for f in fields])
        for filter in (0, 1):
            set_mode(s, filter, 1)
            refused(s, capi.ERR_UNSUPPORTED, text=b"x-slab")      # without FS3D_OPT_OUTPUT_SLABS
        s.set_option(capi.OPT_OUTPUT_SLABS, 1)
        set_mode(s, 0, 1)
    refused(lone, capi.ERR_UNSUPPORTED, entries=("rows", "dev"), text=b"lone x-slab")
    refused(lone, capi.ERR_UNSUPPORTED, entries=("get_layer",), text=b"x-slab")
    refused(grp.solvers[1], capi.ERR_UNSUPPORTED, entries=("get_layer",), text=b"x-slab")
    lone.close()
    grp.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_option_at_zero_leaves_every_record_as_it_was(built, dtype):
    dims = (13, 11, 10)
    nodes = make_nodes(dims, GENERAL)
    fields = general_fields(dims, dtype, 38)
    modes = [(0, 0), (1, 0), (0, 1), (1, 1)]

    def records(s):
        out = []
        for filter, vector in modes:
            s.set_option(capi.OPT_OUTPUT_FILTER, filter)
            s.set_option(capi.OPT_OUTPUT_VECTOR, vector)
            for outdims in ((0, 0, 0), COARSE):
                V, T = s.GetLayer(outdims)
                out.append(V.tobytes() + T.tobytes())
        return out
    never = solver_with_next(nodes, dtype, fields)
    want = records(never)
    info = never.get_layer_info()
    never.close()
    s = solver_with_next(nodes, dtype, fields)
    s.set_option(capi.OPT_OUTPUT_GRADIENT, 0)
    assert records(s) == want
    set_mode(s, 1, 1)
    V, _ = s.GetLayer(COARSE)
    assert V.tobytes() not in [w[:V.nbytes] for w in want], "the option is seen"
    s.set_option(capi.OPT_OUTPUT_GRADIENT, 0)
    assert records(s) == want and s.get_layer_info() == info
    s.close()
