"""Result output on the device (k_get_layer, csrc/kernels_output.hip; fs3d_get_layer_rows / _dev / _info; fs3d_get_layer through the same kernel).

FilterToArrays is a gather, so every comparison is array_equal.  `next` is filled through upload_layer with distinct values in a
random order (no time step is needed), the expectation is the numpy gather of download_layer(LAYER_NEXT) taken AFTER the call --
the 99999 stamp on the NODE_OUT cells included."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from cmc_fluid_solver_amd import build as B
from cmc_fluid_solver_amd import capi, grids
from cmc_fluid_solver_amd.slab import out_rows, slab_range

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
INPUTS = os.path.join(HERE, "golden", "inputs")
PARAMS = (200.0, 0.72, 1.4)
DTYPES = [np.float32, np.float64]
SLAB_DIMS = (23, 13, 11)
SLAB_ODX = (4, 23, 0, 50)


def random_fields(shape, dtype, seed):
    """Four fields whose 4*n values are all different (integers + 0.5, exact in fp32 up to 2^23), in a random order."""
    n = int(np.prod(shape))
    assert 4 * n < 1 << 23
    perm = np.random.default_rng(seed).permutation(4 * n)
    return [(perm[v * n:(v + 1) * n] + 0.5).astype(dtype).reshape(shape) for v in range(4)]


def gather(fields, od, x_of_row=None):
    """FilterToArrays (TimeLayer3D.h:819-924) in numpy: out[i, j, k] = f[i*dimx // odx, j*dimy // ody, k*dimz // odz]; x_of_row
    replaces the first index list (a slab: the global source planes less its offset)."""
    dims = fields[0].shape
    idx = [np.arange(o) * d // o for o, d in zip(od, dims)]
    if x_of_row is not None:
        idx[0] = np.asarray(x_of_row, np.int64)
    sel = np.ix_(*idx)
    return np.stack([f[sel] for f in fields[:3]], axis=-1), fields[3][sel].astype(np.float64)


def nan_arrays(od, dtype):
    return np.full(tuple(od) + (3,), np.nan, dtype), np.full(tuple(od), np.nan, np.float64)


def solver_with_next(nodes, dtype, fields):
    s = capi.Solver(nodes, capi.fluid_params(dtype, *PARAMS), dtype)
    s.upload_layer(capi.LAYER_NEXT, fields)
    return s


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("dims", [(37, 29, 22), (40, 36, 32)])
def test_single_context_rows_equal_the_gather_and_get_layer(built, dims, dtype):
    nodes = grids.box_with_obstacle(*dims)
    out_cells = nodes.type == grids.NODE_OUT
    assert out_cells.any() and not out_cells.all()
    fields = random_fields(dims, dtype, 1)
    s = solver_with_next(nodes, dtype, fields)
    dx, dy, dz = dims
    for outdims in ((0, 0, 0), (7, 6, 5), (1, 1, 1), (dx, 5, dz), (3, dy, 64), (50, 41, 37)):
        od = tuple(o or d for o, d in zip(outdims, dims))
        V, T = nan_arrays(od, dtype)
        rows = s.GetLayerRows(V, T, outdims)
        after = s.download_layer(capi.LAYER_NEXT)
        eV, eT = gather(after, od)
        assert rows == (0, od[0]), outdims
        assert np.array_equal(V, eV) and np.array_equal(T, eT), outdims
        gV, gT = s.GetLayer(outdims)
        assert gV.dtype == np.dtype(dtype) and np.array_equal(gV, eV) and np.array_equal(gT, eT), outdims
        # the stamp, and nothing else, has changed `next`
        for f, a in zip(fields, after):
            assert np.array_equal(a[~out_cells], f[~out_cells]) and (a[out_cells] == 99999).all(), outdims
        if outdims == (0, 0, 0):
            assert (T[out_cells] == 99999.0).all() and (V[out_cells] == 99999).all() and (T[~out_cells] != 99999.0).all()
    s.close()


_single = {}


def slab_case(dtype):
    """The SLAB_DIMS grid, its `next` fields and, per odx, the single-context result (computed once per precision)."""
    key = np.dtype(dtype).name
    if key not in _single:
        nodes = grids.box_with_obstacle(*SLAB_DIMS)
        fields = random_fields(SLAB_DIMS, dtype, 2)
        s = solver_with_next(nodes, dtype, fields)
        res = {}
        for odx in SLAB_ODX:
            outdims = (odx, 5, 0)
            od = tuple(o or d for o, d in zip(outdims, SLAB_DIMS))
            V, T = nan_arrays(od, dtype)
            assert s.GetLayerRows(V, T, outdims) == (0, od[0])
            eV, eT = gather(s.download_layer(capi.LAYER_NEXT), od)
            assert np.array_equal(V, eV) and np.array_equal(T, eT)
            V.flags.writeable = T.flags.writeable = False
            res[odx] = (outdims, od, V, T)
        s.close()
        _single[key] = (nodes, fields, res)
    return _single[key]


def bits(a):
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nslabs", [2, 3, 5, 8])
def test_slabs_write_disjoint_rows_of_one_shared_array(built, nslabs, dtype):
    nodes, fields, single = slab_case(dtype)
    gx = SLAB_DIMS[0]
    grp = capi.LocalGroup(nodes, capi.fluid_params(dtype, *PARAMS), nslabs, dtype)
    ranges = [slab_range(gx, r, nslabs) for r in range(nslabs)]
    for s, (x0, x1) in zip(grp.solvers, ranges):
        s.upload_layer(capi.LAYER_NEXT, [f[x0:x1] for f in fields])
    empty = 0
    for odx in SLAB_ODX:
        outdims, od, sV, sT = single[odx]
        # one slab after the other: each writes its rows and nothing else
        V, T = nan_arrays(od, dtype)
        for s, (x0, x1) in zip(grp.solvers, ranges):
            bV, bT = V.copy(), T.copy()
            i0, i1 = s.GetLayerRows(V, T, outdims)
            assert (i0, i1) == out_rows(x0, x1, gx, od[0]), (odx, x0, x1)
            assert np.array_equal(V[i0:i1], sV[i0:i1]) and np.array_equal(T[i0:i1], sT[i0:i1]), (odx, x0, x1)
            for a, b in ((V, bV), (T, bT)):
                assert np.array_equal(bits(a[:i0]), bits(b[:i0])) and np.array_equal(bits(a[i1:]), bits(b[i1:])), (odx, x0, x1)
            empty += i0 == i1
        assert np.array_equal(V, sV) and np.array_equal(T, sT) and not np.isnan(V).any() and not np.isnan(T).any(), odx
        # all slab threads at once, as the driver's GPU n mode calls it
        V, T = nan_arrays(od, dtype)
        got = grp.run(lambda r, s: s.GetLayerRows(V, T, outdims))
        assert got == [out_rows(x0, x1, gx, od[0]) for x0, x1 in ranges], odx
        assert np.array_equal(V, sV) and np.array_equal(T, sT), odx
    assert empty > 0 or nslabs < 5               # 8 slabs, 4 rows: some slabs own none
    # fs3d_get_layer on a slab keeps sampling the slab's own planes
    for s in grp.solvers[:2]:
        for outdims in ((0, 0, 0), (4, 5, 3)):
            od = tuple(o or d for o, d in zip(outdims, s.dims))
            gV, gT = s.GetLayer(outdims)
            eV, eT = gather(s.download_layer(capi.LAYER_NEXT), od)
            assert np.array_equal(gV, eV) and np.array_equal(gT, eT), outdims
    grp.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_device_destination_gets_the_owned_rows_only(built, dtype):
    import torch
    nodes, fields, single = slab_case(dtype)
    gx = SLAB_DIMS[0]
    td = torch.float32 if dtype == np.float32 else torch.float64
    grp = capi.LocalGroup(nodes, capi.fluid_params(dtype, *PARAMS), 3, dtype)
    one = solver_with_next(nodes, dtype, fields)
    ranges = [slab_range(gx, r, 3) for r in range(3)] + [(0, gx)]
    for s, (x0, x1) in zip(grp.solvers, ranges):
        s.upload_layer(capi.LAYER_NEXT, [f[x0:x1] for f in fields])
    for odx in (4, 50):
        outdims, od, sV, sT = single[odx]
        for s, (x0, x1) in zip(grp.solvers + [one], ranges):
            dV = torch.full(od + (3,), -7.0, dtype=td, device="cuda")
            dT = torch.full(od, -7.0, dtype=torch.float64, device="cuda")
            torch.cuda.synchronize()
            i0, i1 = s.GetLayerDev(dV, dT, outdims)
            s.synchronize()
            assert (i0, i1) == out_rows(x0, x1, gx, od[0])
            info = s.get_layer_info()
            assert info["samples"] == (i1 - i0) * od[1] * od[2] and info["bytes_to_host"] == 0
            hV, hT = dV.cpu().numpy(), dT.cpu().numpy()
            assert np.array_equal(hV[i0:i1], sV[i0:i1]) and np.array_equal(hT[i0:i1], sT[i0:i1]), (odx, x0, x1)
            for h in (hV, hT):
                assert (h[:i0] == -7.0).all() and (h[i1:] == -7.0).all(), (odx, x0, x1)
            # raw pointers are taken as well
            assert s.GetLayerDev(dV.data_ptr(), dT.data_ptr(), outdims) == (i0, i1)
            s.synchronize()
            assert np.array_equal(dV.cpu().numpy(), hV) and np.array_equal(dT.cpu().numpy(), hT)
    with pytest.raises(ValueError):
        one.GetLayerDev(torch.zeros(5, dtype=td, device="cuda"), torch.zeros(5, dtype=torch.float64, device="cuda"), (4, 5, 0))
    one.close()
    grp.close()


@pytest.mark.parametrize("dtype,nbytes", [(np.float32, 4200), (np.float64, 6720)])
def test_get_layer_info_counts_samples_bytes_and_allocations(built, dtype, nbytes):
    dims = (37, 29, 22)
    nodes = grids.box_with_obstacle(*dims)
    s = solver_with_next(nodes, dtype, random_fields(dims, dtype, 3))
    assert s.get_layer_info() == {"samples": 0, "bytes_to_host": 0, "device_allocs": 0}
    V, T = nan_arrays((7, 6, 5), dtype)
    s.GetLayerRows(V, T, (7, 6, 5))
    first = s.get_layer_info()
    assert first == {"samples": 210, "bytes_to_host": nbytes, "device_allocs": 1}
    s.GetLayerRows(V, T, (7, 6, 5))
    s.GetLayer((7, 6, 5))
    s.GetLayer((3, 2, 5))                                      # smaller: the staging buffer holds it
    assert s.get_layer_info() == {"samples": 30, "bytes_to_host": nbytes // 7, "device_allocs": 1}
    s.GetLayer()                                               # larger: it grows, once
    n = int(np.prod(dims))
    assert s.get_layer_info() == {"samples": n, "bytes_to_host": n * (nbytes // 210), "device_allocs": 2}
    s.GetLayer()
    s.GetLayerRows(V, T, (7, 6, 5))
    assert s.get_layer_info() == {"samples": 210, "bytes_to_host": nbytes, "device_allocs": 2}
    s.close()


@pytest.mark.parametrize("filter", [0, 1])
def test_a_larger_record_of_a_time_statistic_counts_its_one_allocation(built, filter):
    """Two buffers serve a record of a statistic layer, the staging buffer and the layer: a larger record grows the first and finds
    the second as it is -- one allocation more, through the gather and through the box kernel."""
    nodes = grids.box_with_obstacle(23, 13, 11)
    s = capi.Solver(nodes, capi.fluid_params(np.float32, 200.0, 0.72, 1.4), np.float32)
    s.set_option(capi.OPT_TIME_STATS, 1)
    s.UpdateBoundaries()
    s.TimeStep(0.05, 1, 1, True)
    s.set_option(capi.OPT_OUTPUT_SOURCE, 1)
    s.set_option(capi.OPT_OUTPUT_FILTER, filter)
    allocs = []
    for od in ((5, 4, 7), (5, 4, 7), (0, 0, 0), (0, 0, 0), (5, 4, 7)):
        s.GetLayer(od)
        allocs.append(s.get_layer_info()["device_allocs"])
    assert allocs == [2, 2, 3, 3, 3]
    s.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_refusals_leave_the_context_usable(built, dtype):
    dims = (12, 9, 10)
    nodes = grids.box_with_obstacle(*dims)
    s = solver_with_next(nodes, dtype, random_fields(dims, dtype, 4))
    lib, od = s.lib, (5, 4, 3)
    V, T = nan_arrays(od, dtype)
    pV, pT = V.ctypes.data_as(C.c_void_p), T.ctypes.data_as(C.c_void_p)
    rows = (C.c_int * 2)(-1, -1)
    for bad in ((-1, 4, 3), (5, -4, 3), (5, 4, -3)):
        assert lib.fs3d_get_layer(s.h, pV, pT, *bad) == capi.ERR_INVALID
        assert lib.fs3d_get_layer_rows(s.h, pV, pT, *bad, rows) == capi.ERR_INVALID
        assert lib.fs3d_get_layer_dev(s.h, pV, pT, *bad, rows) == capi.ERR_INVALID      # refused before the pointers are used
    for fn in (lib.fs3d_get_layer_rows, lib.fs3d_get_layer_dev):
        assert fn(s.h, None, pT, *od, rows) == capi.ERR_INVALID
        assert fn(s.h, pV, None, *od, rows) == capi.ERR_INVALID
        assert fn(s.h, pV, pT, *od, None) == capi.ERR_INVALID
        assert fn(None, pV, pT, *od, rows) == capi.ERR_INVALID
    assert lib.fs3d_get_layer(s.h, None, pT, *od) == capi.ERR_INVALID and lib.fs3d_get_layer(s.h, pV, None, *od) == capi.ERR_INVALID
    assert lib.fs3d_get_layer_info(s.h, None) == capi.ERR_INVALID
    assert np.isnan(V).all() and np.isnan(T).all() and list(rows) == [-1, -1]
    # a context without nodes
    h = C.c_void_p()
    assert lib.fs3d_create(C.byref(h), 0, s.prec, *dims, 0.1, 0.1, 0.1, 0, dims[0]) == capi.OK
    assert lib.fs3d_get_layer(h, pV, pT, *od) == capi.ERR_INVALID
    assert lib.fs3d_get_layer_rows(h, pV, pT, *od, rows) == capi.ERR_INVALID
    assert lib.fs3d_get_layer_dev(h, pV, pT, *od, rows) == capi.ERR_INVALID
    assert b"upload nodes first" in lib.fs3d_last_error(h)
    lib.fs3d_destroy(h)
    # the refused context goes on
    assert s.GetLayerRows(V, T, od) == (0, 5)
    eV, eT = gather(s.download_layer(capi.LAYER_NEXT), od)
    assert np.array_equal(V, eV) and np.array_equal(T, eT)
    s.close()


@pytest.mark.parametrize("mode", [["GPU"], ["GPU", "2", "--same-device"]])
def test_driver_time_output_line_counts_the_records(built, mode, tmp_path):
    from scipy.io import netcdf_file
    driver = B.build_driver()
    data, cfgf = (os.path.join(INPUTS, f) for f in ("box_pipe_2D_data.txt", "box_pipe_2D_config.txt"))
    prefix = str(tmp_path / "box")
    out = subprocess.run([driver, data, prefix, cfgf, "align"] + mode + ["--steps", "12", "--time-output"], check=True, capture_output=True,
                         text=True, timeout=300).stdout
    m = re.findall(r"^Result output per record \(host clock, ms\): GetLayer ([0-9.]+), AppendLayer ([0-9.]+); (\d+) records$", out, re.M)
    assert len(m) == 1, out[-600:]
    f = netcdf_file(prefix + "_res.nc", "r", mmap=False)
    nrec = f.variables["u"].shape[0]
    f.close()
    assert int(m[0][2]) == nrec >= 1 and float(m[0][0]) > 0
    assert out.rstrip().splitlines()[-1].startswith("12 steps in ")
    # without the word the line is absent
    out = subprocess.run([driver, data, prefix, cfgf, "align"] + mode + ["--steps", "2"], check=True, capture_output=True, text=True, timeout=300).stdout
    assert "Result output per record" not in out
