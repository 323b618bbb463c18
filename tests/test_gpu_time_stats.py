"""Time statistics on the device (csrc/kernels_stats.hip: FS3D_OPT_TIME_STATS, FS3D_OPT_OUTPUT_SOURCE) against their numpy twin
(cmc_fluid_solver_amd/time_stats.py).

Every comparison is array_equal (NaN equal to NaN: the sign of a NaN an invalid operation makes is the machine's).  The twin is fed
the `cur` downloaded after each step of the same context, so the rounding of the sweeps plays no part and the default kernels serve.
A step is one of three kinds: `real` (UpdateBoundaries, one ADI step), `fresh` (a random `cur` near 1 uploaded first, then real),
and `wild` (fields spanning 1e-20 .. 1e20 uploaded into `next`, then a step of zero iterations, which only swaps: `cur` then holds the
wild fields, so wide exponents reach the accumulators without a sweep ever reading them).
The expected record is the twin's Q, the 99999 stamp on the NODE_OUT cells, and the numpy gather of test_gpu_get_layer.py."""
import ctypes as C

import numpy as np
import pytest

from cmc_fluid_solver_amd import capi, grids
from cmc_fluid_solver_amd import layer_output as LO
from cmc_fluid_solver_amd import time_stats as TS
from cmc_fluid_solver_amd.slab import out_rows, slab_range

pytestmark = pytest.mark.gpu

PARAMS = (200.0, 0.72, 1.4)
DT = 0.1
DTYPES = [np.float32, np.float64]
COARSE = (7, 6, 5)
SLAB_DIMS = (23, 13, 11)
PLAN = ("real", "wild", "fresh", "real", "wild", "fresh")


def gather(fields, od, x_of_row=None):
    """FilterToArrays (TimeLayer3D.h:819-924) in numpy: out[i, j, k] = f[i*dimx // odx, j*dimy // ody, k*dimz // odz]"""
    dims = fields[0].shape
    idx = [np.arange(o) * d // o for o, d in zip(od, dims)]
    if x_of_row is not None:
        idx[0] = np.asarray(x_of_row, np.int64)
    sel = np.ix_(*idx)
    return np.stack([f[sel] for f in fields[:3]], axis=-1), fields[3][sel].astype(np.float64)


def nan_arrays(od, dtype):
    return np.full(tuple(od) + (3,), np.nan, dtype), np.full(tuple(od), np.nan, np.float64)


def same(a, b):
    return a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True)


def wide_fields(rng, shape, dtype):
    return [(rng.choice([-1.0, 1.0], shape) * 10.0 ** rng.uniform(-20, 20, shape)).astype(dtype) for _ in range(4)]


def near_one(rng, shape, dtype, nodes):
    base = [np.asarray(a, dtype) for a in (nodes.vx, nodes.vy, nodes.vz, nodes.T)]
    return [(b + rng.uniform(-0.05, 0.05, shape)).astype(dtype) for b in base]


def do_step(s, kind, rng, nodes, use_async=False):
    """One step of the given kind on context s; returns the `cur` it leaves"""
    if kind == "wild":
        s.upload_layer(capi.LAYER_NEXT, wide_fields(rng, s.dims, s.dtype))
        s.TimeStep(DT, 0, 0, False)
    else:
        if kind == "fresh":
            s.upload_layer(capi.LAYER_CUR, near_one(rng, s.dims, s.dtype, nodes))
        if use_async:
            s.time_step_async(DT, 1, 1)
            s.synchronize()
        else:
            s.UpdateBoundaries()
            s.TimeStep(DT, 1, 1, False)
    return s.download_layer(capi.LAYER_CUR)


def expected(twin, source, cur, types, od):
    return gather(LO.stamp(types, twin.layer(source, cur)), od)


def check_sources(s, twin, types, sources, outdims=((0, 0, 0), COARSE), what=""):
    cur = s.download_layer(capi.LAYER_CUR)
    for source in sources:
        s.set_option(capi.OPT_OUTPUT_SOURCE, source)
        for outdims_ in outdims:
            od = tuple(o or d for o, d in zip(outdims_, s.dims))
            eV, eT = expected(twin, source, cur, types, od)
            V, T = s.GetLayer(outdims_)
            assert same(V, eV) and same(T, eT), (what, source, outdims_)
    s.set_option(capi.OPT_OUTPUT_SOURCE, 0)


class DeviceArray:
    """A host array's copy in device memory of device 0, through the HIP runtime the library runs on (fs3d_get_layer_dev takes raw
    pointers)"""
    _hip = None

    def __init__(self, host):
        if DeviceArray._hip is None:
            hip = C.CDLL("libamdhip64.so")
            hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
            hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
            hip.hipFree.argtypes = [C.c_void_p]
            DeviceArray._hip = hip
        self.host = np.ascontiguousarray(host)
        p = C.c_void_p()
        assert self._hip.hipMalloc(C.byref(p), self.host.nbytes) == 0
        self.ptr = p.value
        assert self._hip.hipMemcpy(self.ptr, self.host.ctypes.data, self.host.nbytes, 1) == 0      # hipMemcpyHostToDevice

    def download(self):
        out = np.empty_like(self.host)
        assert self._hip.hipMemcpy(out.ctypes.data, self.ptr, out.nbytes, 2) == 0                   # hipMemcpyDeviceToHost
        return out

    def free(self):
        self._hip.hipFree(self.ptr)


def obstacle(dims, lo=0.25, hi=0.7):
    """box_with_obstacle with a block wide enough to hold NODE_OUT cells on these small grids"""
    return grids.box_with_obstacle(*dims, lo=lo, hi=hi)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("dims", [(16, 12, 8), (9, 7, 5), (4, 7, 5), (40, 36, 32)])
def test_sources_equal_the_twin_on_every_launch_form(built, dims, mode, dtype):
    """16 x 12 x 8: the vector form; 9 x 7 x 5: 315 cells, cell by cell (an odd count, planes of 35); 4 x 7 x 5: 140 cells, a
    multiple of 4 whose fields start a plane of 35 elements into their buffer, off the 16 bytes: cell by cell too; 40 x 36 x 32: 45
    workgroups"""
    # (five cells along z hold no block that is more than one cell thick, which the tables refuse: the plain box there)
    nodes = obstacle(dims) if dims[2] != 5 else grids.box(*dims)
    types = np.asarray(nodes.type)
    if dims[2] != 5:
        assert (types == grids.NODE_OUT).any()
    assert (types == grids.NODE_IN).any() and (types == grids.NODE_BOUND).any()
    s = capi.Solver(nodes, capi.fluid_params(dtype, *PARAMS), dtype)
    s.set_option(capi.OPT_TIME_STATS, mode)
    twin = TS.TimeStats(dims, mode)
    rng = np.random.default_rng(11)
    for kind in PLAN:
        twin.add(do_step(s, kind, rng, nodes), types)
    before = s.download_layer(capi.LAYER_CUR), s.download_layer(capi.LAYER_NEXT)
    check_sources(s, twin, types, (1, 2, 3) if mode == 2 else (1, 3), what=dims)
    # `cur` and `next` are bit-identical around the calls, and the usual counts are reported
    after = s.download_layer(capi.LAYER_CUR), s.download_layer(capi.LAYER_NEXT)
    for a, b in zip(before[0] + before[1], after[0] + after[1]):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    s.set_option(capi.OPT_OUTPUT_SOURCE, 3)
    V, T = nan_arrays(COARSE, dtype)
    assert s.GetLayerRows(V, T, COARSE) == (0, COARSE[0])
    info = s.get_layer_info()
    assert info["samples"] == 210 and info["bytes_to_host"] == 210 * (3 * np.dtype(dtype).itemsize + 8)
    eV, eT = expected(twin, 3, after[0], types, COARSE)
    assert same(V, eV) and same(T, eT)
    assert (V[T != 99999.0] == 0).all() and ((T >= 0) & (T <= 1) | (T == 99999.0)).all()
    s.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_option_off_changes_nothing_and_allocates_nothing(built, dtype):
    """The accumulators go through the counter of fs3d_geometry_info entry 13: it stands still while the option is 0."""
    dims = (16, 12, 8)
    nodes = obstacle(dims)
    results, allocs = [], []
    for mode in (0, 2):
        s = capi.Solver(nodes, capi.fluid_params(dtype, *PARAMS), dtype)
        a0 = s.geometry_info()["device_allocs_and_frees"]
        s.set_option(capi.OPT_TIME_STATS, mode)
        for _ in range(4):
            s.UpdateBoundaries()
            s.TimeStep(DT, 2, 1, True)
        results.append(s.download_layer(capi.LAYER_CUR) + s.download_layer(capi.LAYER_NEXT))
        allocs.append(s.geometry_info()["device_allocs_and_frees"] - a0)
        if mode:
            s.set_option(capi.OPT_TIME_STATS, 0)               # frees the three accumulators
            assert s.geometry_info()["device_allocs_and_frees"] - a0 == 6
            s.UpdateBoundaries()
            s.TimeStep(DT, 2, 1, True)
            assert s.geometry_info()["device_allocs_and_frees"] - a0 == 6
        s.close()
    assert allocs == [0, 3]
    for a, b in zip(*results):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))


@pytest.mark.parametrize("dtype", DTYPES)
def test_setting_the_option_opens_a_new_window_and_async_steps_accumulate(built, dtype):
    dims = (16, 12, 8)
    nodes = obstacle(dims)
    types = np.asarray(nodes.type)
    s = capi.Solver(nodes, capi.fluid_params(dtype, *PARAMS), dtype)
    s.set_option(capi.OPT_TIME_STATS, 2)
    rng = np.random.default_rng(12)
    for kind in PLAN[:3]:
        do_step(s, kind, rng, nodes)
    s.set_option(capi.OPT_TIME_STATS, 2)                       # the same value: still a new window
    twin = TS.TimeStats(dims, 2)
    for k, kind in enumerate(PLAN[3:]):
        twin.add(do_step(s, kind, rng, nodes, use_async=k != 1), types)
    assert twin.N == 3
    check_sources(s, twin, types, (1, 2, 3), what="steps 4..6")
    # mode 2 -> 1 without passing 0: a new window again, and the variance is no longer held
    s.set_option(capi.OPT_TIME_STATS, 1)
    twin = TS.TimeStats(dims, 1)
    twin.add(do_step(s, "real", rng, nodes, use_async=True), types)
    check_sources(s, twin, types, (1, 3), outdims=(COARSE,), what="mode 1")
    s.close()


def test_a_diverged_step_accumulates_nothing(built):
    """grids.perturb(.., vel=50) on the 12 x 9 x 10 box: the CPU path reports diffError 8.6 > 0.01 (checked here with the oracle)."""
    from oracle import oracle as O
    dtype, dims = np.float32, (12, 9, 10)
    nodes = grids.box_with_obstacle(*dims, h=0.04)
    types = np.asarray(nodes.type)
    params = capi.fluid_params(dtype, *PARAMS)
    base = [np.ascontiguousarray(a, dtype) for a in (nodes.vx, nodes.vy, nodes.vz, nodes.T)]
    wild = grids.perturb(base, vel=50.0)
    o = O.Oracle(nodes, params, dtype)
    for v in range(4):
        o.set_field(capi.LAYER_CUR, v, wild[v])
    rc, err = o.time_step(DT, 1, 1, True)
    o.close()
    assert rc != 0 and err > 0.01, "the CPU path diverges on this input"
    s = capi.Solver(nodes, params, dtype)
    s.set_option(capi.OPT_SWEEP_KERNEL, capi.SWEEP_EXACT)
    s.set_option(capi.OPT_TIME_STATS, 2)
    twin = TS.TimeStats(dims, 2)
    for _ in range(2):
        s.UpdateBoundaries()
        s.TimeStep(DT, 1, 1, True)
        twin.add(s.download_layer(capi.LAYER_CUR), types)
    sane = s.download_layer(capi.LAYER_CUR)
    s.upload_layer(capi.LAYER_CUR, wild)
    with pytest.raises(capi.Fs3dError) as ei:
        s.TimeStep(DT, 1, 1, True)
    assert ei.value.status == capi.ERR_DIVERGED
    assert all(np.array_equal(a, b) for a, b in zip(s.download_layer(capi.LAYER_CUR), wild)), "no swap"
    assert twin.N == 2
    check_sources(s, twin, types, (1, 2, 3), what="after the diverged step")      # the fraction: n / 2, not n / 3
    s.upload_layer(capi.LAYER_CUR, sane)
    s.UpdateBoundaries()
    s.TimeStep(DT, 1, 1, True)
    twin.add(s.download_layer(capi.LAYER_CUR), types)
    check_sources(s, twin, types, (1, 2, 3), outdims=(COARSE,), what="the window goes on")
    s.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_moving_geometry_counts_cells_by_their_type_at_each_step(built, dtype):
    dims = (16, 12, 10)
    A, B = obstacle(dims, 0.25, 0.55), obstacle(dims, 0.45, 0.75)
    tA, tB = np.asarray(A.type), np.asarray(B.type)
    inA, inB = tA == grids.NODE_IN, tB == grids.NODE_IN
    assert (inA & ~inB).any() and (inB & ~inA).any() and (inA & inB).any() and (~inA & ~inB).any()
    s = capi.Solver(A, capi.fluid_params(dtype, *PARAMS), dtype)
    s.set_option(capi.OPT_TIME_STATS, 2)
    twin = TS.TimeStats(dims, 2)
    for step in range(6):
        nodes = B if step % 2 else A
        if step:
            s.update_nodes(nodes)
        s.UpdateBoundaries()
        s.TimeStep(DT, 1, 1, False)
        twin.add(s.download_layer(capi.LAYER_CUR), np.asarray(nodes.type))
    assert np.array_equal(twin.n, 3 * inA.astype(np.uint32) + 3 * inB.astype(np.uint32))
    s.set_option(capi.OPT_OUTPUT_SOURCE, 3)
    V, T = s.GetLayer()
    out_now = tB == grids.NODE_OUT                             # the last geometry is B: its NODE_OUT cells carry the stamp
    want = np.where(inA & inB, 1.0, np.where(inA | inB, 0.5, 0.0))
    assert np.array_equal(T[~out_now], want[~out_now]) and (T[out_now] == 99999.0).all()
    assert (V[~out_now] == 0).all()
    assert (T == 0.5).any() and (T == 1.0).any() and (T == 0.0).any()
    # the mean on the cells that were fluid in only some steps
    s.set_option(capi.OPT_OUTPUT_SOURCE, 1)
    V, T = s.GetLayer()
    eV, eT = expected(twin, 1, s.download_layer(capi.LAYER_CUR), tB, dims)
    some = (inA ^ inB) & ~out_now
    assert some.any() and same(V[some], eV[some]) and same(T[some], eT[some])
    check_sources(s, twin, tB, (1, 2, 3), what="moving")
    s.close()


_single = {}


def slab_case(dtype):
    """SLAB_DIMS, exact kernels, 4 steps from a perturbed start: the single context's records of sources 1..3 (once per precision)"""
    key = np.dtype(dtype).name
    if key not in _single:
        nodes = grids.box_with_obstacle(*SLAB_DIMS)
        base = [np.ascontiguousarray(a, dtype) for a in (nodes.vx, nodes.vy, nodes.vz, nodes.T)]
        start = grids.perturb(base, seed=8)
        s = capi.Solver(nodes, capi.fluid_params(dtype, *PARAMS), dtype)
        s.set_option(capi.OPT_SWEEP_KERNEL, capi.SWEEP_EXACT)
        s.set_option(capi.OPT_TIME_STATS, 2)
        s.upload_layer(capi.LAYER_CUR, start)
        twin = TS.TimeStats(SLAB_DIMS, 2)
        for _ in range(4):
            s.UpdateBoundaries()
            s.TimeStep(DT, 2, 1, True)
            twin.add(s.download_layer(capi.LAYER_CUR), nodes.type)
        cur = s.download_layer(capi.LAYER_CUR)
        res = {}
        for source in (1, 2, 3):
            s.set_option(capi.OPT_OUTPUT_SOURCE, source)
            for outdims in ((0, 0, 0), (4, 5, 0), (50, 5, 3)):
                od = tuple(o or d for o, d in zip(outdims, SLAB_DIMS))
                V, T = nan_arrays(od, dtype)
                assert s.GetLayerRows(V, T, outdims) == (0, od[0])
                eV, eT = expected(twin, source, cur, np.asarray(nodes.type), od)
                assert same(V, eV) and same(T, eT)
                V.flags.writeable = T.flags.writeable = False
                res[source, outdims] = (od, V, T)
        s.close()
        _single[key] = (nodes, start, res)
    return _single[key]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nslabs", [2, 3])
def test_slabs_write_the_rows_of_the_single_contexts_record(built, nslabs, dtype):
    nodes, start, single = slab_case(dtype)
    gx = SLAB_DIMS[0]
    grp = capi.LocalGroup(nodes, capi.fluid_params(dtype, *PARAMS), nslabs, dtype)
    ranges = [slab_range(gx, r, nslabs) for r in range(nslabs)]

    def steps(r, sv):
        x0, x1 = ranges[r]
        sv.set_option(capi.OPT_SWEEP_KERNEL, capi.SWEEP_EXACT)      # bit-equal to the single context, cross-slab X solve included
        sv.set_option(capi.OPT_TIME_STATS, 2)
        sv.upload_layer(capi.LAYER_CUR, [f[x0:x1] for f in start])
        for _ in range(4):
            sv.UpdateBoundaries()
            sv.TimeStep(DT, 2, 1, True)
    grp.run(steps)
    for (source, outdims), (od, sV, sT) in single.items():
        V, T = nan_arrays(od, dtype)

        def rows(r, sv):
            sv.set_option(capi.OPT_OUTPUT_SOURCE, source)
            return sv.GetLayerRows(V, T, outdims)
        got = grp.run(rows)
        assert got == [out_rows(x0, x1, gx, od[0]) for x0, x1 in ranges], (source, outdims)
        assert same(V, sV) and same(T, sT), (source, outdims)
    # fs3d_get_layer on a slab samples the slab's own planes of the statistic layer; the device destination gets the same rows
    od, sV, sT = single[1, (0, 0, 0)]
    for sv, (x0, x1) in zip(grp.solvers, ranges):
        sv.set_option(capi.OPT_OUTPUT_SOURCE, 1)
        gV, gT = sv.GetLayer()
        assert same(gV, sV[x0:x1]) and same(gT, sT[x0:x1])
        dV, dT = DeviceArray(np.full(od + (3,), -7.0, dtype)), DeviceArray(np.full(od, -7.0, np.float64))
        assert sv.GetLayerDev(dV.ptr, dT.ptr) == (x0, x1)
        sv.synchronize()
        hV, hT = dV.download(), dT.download()
        assert same(hV[x0:x1], sV[x0:x1]) and same(hT[x0:x1], sT[x0:x1])
        assert (hT[:x0] == -7.0).all() and (hT[x1:] == -7.0).all() and (hV[:x0] == -7.0).all() and (hV[x1:] == -7.0).all()
        dV.free()
        dT.free()
    # the filter on a slab is refused as ever, whatever the source
    sv = grp.solvers[0]
    sv.set_option(capi.OPT_OUTPUT_FILTER, 1)
    V, T = nan_arrays(COARSE, dtype)
    rows_ = (C.c_int * 2)(-1, -1)
    pV, pT = V.ctypes.data_as(C.c_void_p), T.ctypes.data_as(C.c_void_p)
    assert sv.lib.fs3d_get_layer_rows(sv.h, pV, pT, *COARSE, rows_) == capi.ERR_UNSUPPORTED
    assert sv.lib.fs3d_get_layer(sv.h, pV, pT, *COARSE) == capi.ERR_UNSUPPORTED
    assert np.isnan(V).all() and np.isnan(T).all() and list(rows_) == [-1, -1]
    grp.close()


def exact_fields(shape, dtype, seed):
    """Four fields of distinct integers + 0.5 in a random order: sums of a few hundred of them are exact in fp32 and in double"""
    n = int(np.prod(shape))
    perm = np.random.default_rng(seed).permutation(4 * n)
    return [(perm[v * n:(v + 1) * n] + 0.5).astype(dtype).reshape(shape) for v in range(4)]


@pytest.mark.parametrize("dtype", DTYPES)
def test_filter_and_vorticity_run_on_the_mean(built, dtype):
    """Four steps of integers + 0.5: every mean is a multiple of 1/8 below 2^20, so the box sums of the filter are exact and the
    kernel equals layer_output.py's rule bit for bit; the curl is per cell in R, bit for bit by itself."""
    dims = (16, 12, 8)
    nodes = obstacle(dims)
    types = np.asarray(nodes.type)
    s = capi.Solver(nodes, capi.fluid_params(dtype, *PARAMS), dtype)
    s.set_option(capi.OPT_TIME_STATS, 1)
    twin = TS.TimeStats(dims, 1)
    for k in range(4):
        s.upload_layer(capi.LAYER_NEXT, exact_fields(dims, dtype, 20 + k))
        s.TimeStep(DT, 0, 0, False)                            # zero iterations: the swap alone
        twin.add(s.download_layer(capi.LAYER_CUR), types)
    cur = s.download_layer(capi.LAYER_CUR)
    Q = twin.layer(1, cur)
    fluid = types == grids.NODE_IN
    assert all((q[fluid] * 8 == np.round(q[fluid] * 8)).all() and np.abs(q[fluid]).max() < 2 ** 20 for q in Q)
    spacing = (nodes.dx, nodes.dy, nodes.dz)
    s.set_option(capi.OPT_OUTPUT_SOURCE, 1)
    point = s.GetLayer(COARSE)
    for filt, vec in ((1, 0), (0, 1)):
        s.set_option(capi.OPT_OUTPUT_FILTER, filt)
        s.set_option(capi.OPT_OUTPUT_VECTOR, vec)
        for outdims in (COARSE, (0, 0, 0)):
            V, T = s.GetLayer(outdims)
            eV, eT = LO.layer_output(types, Q, outdims, filt, vec, spacing)
            assert same(V, eV) and same(T, eT), (filt, vec, outdims)
            if outdims == COARSE:
                assert not np.array_equal(V, point[0]), "the option is seen"
    s.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_refusals_leave_destinations_and_context_as_they_were(built, dtype):
    dims = (12, 9, 10)
    nodes = grids.box_with_obstacle(*dims)
    types = np.asarray(nodes.type)
    s = capi.Solver(nodes, capi.fluid_params(dtype, *PARAMS), dtype)
    lib = s.lib
    for opt, bad in ((capi.OPT_TIME_STATS, (-1, 3, 7)), (capi.OPT_OUTPUT_SOURCE, (-1, 4, 9))):
        for v in bad:
            assert lib.fs3d_set_option(s.h, opt, v) == capi.ERR_INVALID
            assert lib.fs3d_last_error(s.h)
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
    for source in (1, 2, 3):                                   # any source while the option is 0
        s.set_option(capi.OPT_OUTPUT_SOURCE, source)
        refused("mode 0, source %d" % source)
    s.set_option(capi.OPT_TIME_STATS, 1)
    for source in (1, 2, 3):                                   # N = 0
        s.set_option(capi.OPT_OUTPUT_SOURCE, source)
        refused("no step yet, source %d" % source)
    assert b"no time step" in lib.fs3d_last_error(s.h)
    twin = TS.TimeStats(dims, 1)
    for _ in range(2):
        s.UpdateBoundaries()
        s.TimeStep(DT, 1, 1, True)
        twin.add(s.download_layer(capi.LAYER_CUR), types)
    s.set_option(capi.OPT_OUTPUT_SOURCE, 2)                    # the variance in mode 1
    refused("mode 1, source 2")
    assert b"variance" in lib.fs3d_last_error(s.h)
    # the refused context goes on: sources 1 and 3, one more step, source 0 as ever
    check_sources(s, twin, types, (1, 3), outdims=(COARSE,))
    s.UpdateBoundaries()
    s.TimeStep(DT, 1, 1, True)
    twin.add(s.download_layer(capi.LAYER_CUR), types)
    check_sources(s, twin, types, (1, 3), outdims=(COARSE,))
    gV, gT = s.GetLayer(COARSE)
    eV, eT = gather(s.download_layer(capi.LAYER_NEXT), COARSE)
    assert same(gV, eV) and same(gT, eT)
    s.close()
