"""Open fluid runs and NODE_IN START rows on the GPU, through the C ABI: the grids of tests/open_run_cases.py (their CPU
conditions: tests/test_open_run_cases.py) against the CPU oracle.

A NODE_IN cell on no segment of a direction is written by no sweep of it; the merge averages the STALE value of the sweep's
output layer into temp there.  Every path has code of its own for it: the thread-per-line and pipelined kernels re-read `next` on
ROW_SKIP cells, the X/Y and Z partition kernels have a branch that loads it, and the fused time step drops the `next` store of an
iteration-closing X sweep only where stale_in_cells == 0.  All four layers are seeded (open_run_cases.seed_all): the stale values
of the first step are then the same on both sides, and on the cases flagged sensitive the oracle's answer depends on them.

    bit-exact kernels (LINE, PIPE; fp32 and fp64)    equal to the oracle value for value: sweeps, and cur / next / temp, GetLayer
                                                     after every step; diffError to 1e-12 relative (its summation order differs)
    partition kernels, one merged sweep              the written cells are the reference's; the merged temp of a stale cell is
                                                     (temp + next) / 2 of uploaded values: BIT-EQUAL; next elsewhere rel-L2 <=
                                                     TOL_SWEEP of tests/test_gpu_part.py (fp64: of tests/test_gpu_part_f64.py);
                                                     merged temp elsewhere: |dT| = |dnext| / 2 plus one rounding of the average,
                                                     ||dT|| <= TOL_SWEEP / 2 ||next|| + eps ||T||
    partition kernels, 3 steps (G 4, L 2)            assert_step_close with TOL_STEPS of the same two files; where the oracle's own
                                                     fp32 result is further than TOL_STEPS from its fp64 result on the case (decided
                                                     on the CPU), ALSO the _yardstick rule of tests/test_gpu_part.py: at most
                                                     1.5 x the sequential fp32 deviation from the fp64 solution.
    x-slabs                                          exact kernels: the single context's and the oracle's bits; the default
                                                     (reduced-interface X solve): the partition bound above
    a geometry that opens and closes                 update_nodes(_dev) == a fresh context on the target geometry bit for bit;
                                                     exact kernels also == the oracle driven through the same geometries

The distances measured on one MI355X are in DESIGN.md section 5, each beside its closed twin's (the same grid, windows shut).
"""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if os.path.dirname(HERE) not in sys.path:          # run as a script (the child processes below)
    sys.path.insert(0, os.path.dirname(HERE))

import open_run_cases as OC  # noqa: E402
import test_gpu_part as P32  # noqa: E402
import test_gpu_part_f64 as P64  # noqa: E402
from cmc_fluid_solver_amd import capi, grids  # noqa: E402
from cmc_fluid_solver_amd.slab import slab_range  # noqa: E402

pytestmark = pytest.mark.gpu

DT = OC.DT
CTN = (capi.LAYER_CUR, capi.LAYER_TEMP, capi.LAYER_NEXT)
EPS = {"f32": 2.0 ** -24, "f64": 2.0 ** -53}


@pytest.fixture
def exact_default(monkeypatch):
    """New contexts start on the bit-exact kernels (FS3D_SWEEP_EXACT), as in tests/test_gpu_parity.py."""
    monkeypatch.setenv("FS3D_DEFAULT_KERNEL", "4")


def make(name, dtype, kernel=None, fuse=1, keep=None, f64_part=0, closed=False, x_range=None):
    s = capi.Solver(OC.grid(name, closed), capi.fluid_params(dtype, *OC.PARAMS), dtype, x_range=x_range)
    if kernel is not None:
        s.set_option(capi.OPT_SWEEP_KERNEL, kernel)
    s.set_option(capi.OPT_FUSE_MERGE, fuse)
    if keep is not None:
        s.set_option(capi.OPT_KEEP_TEMP, keep)
    if f64_part:
        s.set_option(capi.OPT_F64_PART, f64_part)
    return s


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


def assert_equal(A, B, what):
    for v, (a, b) in enumerate(zip(A, B)):
        if not np.array_equal(a, b):
            bad = np.argwhere(a != b)
            raise AssertionError("%s: field %d differs at %d cells, first %s: hip=%r oracle=%r" % (what, v, len(bad), bad[0], a[tuple(bad[0])], b[tuple(bad[0])]))


def host_stale_count(name):
    """stale_in_cells of the host table builder (tests/test_open_run_cases.py holds the builder to this restatement)."""
    return OC.tables(name)["stale_in_cells"]


# ---- a. exact kernels, one sweep at a time ----------------------------------------------------------------------------------
# (the decorator on top varies fastest: the references of one (case, precision) serve the tests that follow each other)

@pytest.mark.parametrize("d", [0, 1, 2])
@pytest.mark.parametrize("fuse", [0, 1])
@pytest.mark.parametrize("kernel", [capi.SWEEP_LINE, capi.SWEEP_PIPE])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("name", OC.ALL)
def test_exact_sweeps_equal_the_oracle(built, name, dtype, kernel, fuse, d):
    """Two merged sweeps of one direction on the seeded state: the second merges the stale value a second time."""
    want_next, want_temp = OC.merged_sweeps_reference(name, dtype)[d]
    want_kernel = capi.KERNEL_NAMES[kernel]
    s = make(name, dtype, kernel, fuse)
    OC.seed_all(name, s=s)
    try:
        s.sweep(d, DT, *CTN, merge=True)
    except capi.Fs3dError as e:
        # the pipelined kernel refuses Z lines that are no whole number of 16-byte pieces: EXACT must run the thread-per-line walk
        assert e.status == capi.ERR_UNSUPPORTED and kernel == capi.SWEEP_PIPE and d == 2 and OC.grid(name).dimz % 4 != 0, str(e)
        s.set_option(capi.OPT_SWEEP_KERNEL, capi.SWEEP_EXACT)
        want_kernel = "line"
        OC.seed_all(name, s=s)
        s.sweep(d, DT, *CTN, merge=True)
    s.sweep(d, DT, *CTN, merge=True)
    assert s.last_sweep_kernels()["XYZ"[d]] == want_kernel
    assert_equal(s.download_layer(capi.LAYER_NEXT), want_next, "%s dir %d: next" % (name, d))
    assert_equal(s.download_layer(capi.LAYER_TEMP), want_temp, "%s dir %d: merged temp" % (name, d))
    s.close()


# ---- b. exact kernels, whole steps ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("keep", [0, 1])
@pytest.mark.parametrize("fuse", [0, 1])
@pytest.mark.parametrize("GL", [(4, 2), (1, 1), (3, 1), (2, 3)])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("name", OC.ALL)
def test_exact_steps_equal_the_oracle(built, exact_default, name, dtype, GL, fuse, keep):
    """Three steps from the seeded state.  With G >= 2 the fused step may drop the `next` store of the X sweep that closes an
    iteration only on a geometry without stale cells: z_hi, z_through, all_three and the other Z-open cases read it."""
    ref = OC.steps_reference(name, dtype, *GL, get_layers=True)
    s = make(name, dtype, None, fuse, keep)
    assert s.geometry_info()["stale_in_cells"] == host_stale_count(name)          # the device reduction of kernels_geom.hip
    OC.seed_all(name, s=s)
    for step, want in enumerate(ref):
        s.UpdateBoundaries()
        e = s.TimeStep(DT, GL[0], GL[1], True)
        assert want.rc == 0 and e == pytest.approx(want.err, rel=1e-12), "diffError step %d" % step
        assert_equal(s.download_layer(capi.LAYER_CUR), want.cur, "%s: cur after step %d" % (name, step))
        assert_equal(s.download_layer(capi.LAYER_NEXT), want.next, "%s: next after step %d" % (name, step))
        if keep:
            assert_equal(s.download_layer(capi.LAYER_TEMP), want.temp, "%s: temp after step %d" % (name, step))
        for od, (Vo, To) in zip(OC.OUTDIMS, want.layers):
            V, T = s.GetLayer(od)
            assert np.array_equal(V, Vo) and np.array_equal(T, To), "GetLayer%s after step %d" % (od, step)
    assert all(k.split("-")[0] in ("pipe", "line") for k in s.last_sweep_kernels().values()), s.last_sweep_kernels()
    s.close()


# ---- c. partition kernels ---------------------------------------------------------------------------------------------------

PREC = {"f32": (np.float32, 0, P32), "f64": (np.float64, 1, P64)}
PART_SWEEPS = [(n, d) for n in OC.PART for d in range(3) if "XYZ"[d] in OC.CASES[n].part]


def part_sweep(name, prec, d, closed):
    """One merged sweep of direction d with the sentinel in next, against the oracle; returns the largest rel-L2 distance of next
    and of the merged temp off the stale cells."""
    dtype, f64_part, P = PREC[prec]
    g = OC.grid(name, closed)
    want_next, want_temp = OC.sentinel_sweep_reference(name, dtype, closed)[d]
    s = make(name, dtype, capi.SWEEP_PART, f64_part=f64_part, closed=closed)
    OC.seed_all(name, s=s, closed=closed, sentinel_next=True)
    s.sweep(d, DT, *CTN, merge=True)
    assert s.last_sweep_kernels()["XYZ"[d]] == "part"                              # never a silent fallback
    A, T = s.download_layer(capi.LAYER_NEXT), s.download_layer(capi.LAYER_TEMP)
    s.close()
    tmp0 = OC.seeded(name, closed=closed)[capi.LAYER_TEMP]
    fluid = g.type == grids.NODE_IN
    stale = np.zeros(g.shape, bool) if closed else OC.stale_mask(name, d)      # none in the directions a window does not open
    solved = fluid & ~stale
    worst = [0.0, 0.0]
    for v in range(4):
        assert np.isfinite(A[v]).all() and np.isfinite(T[v]).all(), "field %d has non-finite values" % v
        assert np.array_equal(A[v] == OC.SENTINEL, want_next[v] == OC.SENTINEL), "the set of written cells differs from the reference's"
        assert np.array_equal(bits(T[v][stale]), bits(want_temp[v][stale])), "field %d: the merged temp of %d stale cells differs" % (
            v, int((bits(T[v][stale]) != bits(want_temp[v][stale])).sum()))
        assert np.array_equal(bits(T[v][~fluid]), bits(tmp0[v][~fluid].astype(dtype))), "cells that are not NODE_IN are left as they were"
        r = P.rel(A[v], want_next[v])
        far = np.argwhere(np.abs(A[v].astype(np.float64) - want_next[v]) > 256 * EPS[prec] * np.abs(want_next[v]).max())
        if len(far):
            print("%s %s %s field %d: %d cells of next further than 256 eps of the field scale from the oracle, within %s .. %s" % (
                name, prec, "XYZ"[d], v, len(far), far.min(axis=0), far.max(axis=0)))
        dt_norm = float(np.linalg.norm(T[v][solved].astype(np.float64) - want_temp[v][solved]))
        bound_t = 0.5 * P.TOL_SWEEP * float(np.linalg.norm(want_next[v][solved].astype(np.float64))) + \
            EPS[prec] * float(np.linalg.norm(want_temp[v][solved].astype(np.float64)))
        rt = dt_norm / float(np.linalg.norm(want_temp[v][solved].astype(np.float64)))
        worst = [max(worst[0], r), max(worst[1], rt)]
        assert r <= P.TOL_SWEEP, "next after sweep %d: field %d rel-L2 %.2e > %.1e" % (d, v, r, P.TOL_SWEEP)
        assert dt_norm <= bound_t, "merged temp after sweep %d: field %d off by %.3e > %.3e" % (d, v, dt_norm, bound_t)
    return worst


@pytest.mark.parametrize("prec", list(PREC))
@pytest.mark.parametrize("name,d", PART_SWEEPS)
def test_part_sweep_with_a_sentinel_in_next(built, name, d, prec):
    open_, twin = part_sweep(name, prec, d, False), part_sweep(name, prec, d, True)
    print("DIST sweep %s %s %s: next %.2e (closed twin %.2e), merged temp off the stale cells %.2e (closed twin %.2e)" % (
        prec, name, "XYZ"[d], open_[0], twin[0], open_[1], twin[1]))


class _Ref:
    """a recorded oracle state where assert_step_close expects a live oracle"""
    def __init__(self, cur):
        self.cur = cur

    def get_layer_fields(self, layer):
        return self.cur


def oracle_fp32_deviation(name, step, closed=False):
    """How far the oracle's own fp32 result is from its fp64 result after that step (velocity as a vector, T)."""
    a, b = OC.steps_reference(name, np.float32, closed=closed)[step].cur, OC.steps_reference(name, np.float64, closed=closed)[step].cur
    return max(P32.vec_rel(a, b), P32.rel(a[3], b[3]))


def part_step_check(s, name, prec, step, what, closed=False, check=True):
    """cur of context s (or fields) after `step` against the bound of the docstring's third row; returns (velocity, T) distances."""
    dtype, _, P = PREC[prec]
    want = OC.steps_reference(name, dtype, closed=closed)[step].cur
    A = s.download_layer(capi.LAYER_CUR) if hasattr(s, "download_layer") else s
    dist = P.vec_rel(A, want), P.rel(A[3], want[3])
    if not check:
        return dist
    for a in A:
        assert np.isfinite(a).all(), what

    class Fields:
        def download_layer(self, layer):
            return A
    P.assert_step_close(Fields(), _Ref(want), P.TOL_STEPS, what)
    if prec == "f32" and oracle_fp32_deviation(name, step, closed) > P32.TOL_STEPS:
        P32._yardstick(A, want, OC.steps_reference(name, np.float64, closed=closed)[step].cur, what)
    return dist


@pytest.mark.parametrize("prec", list(PREC))
@pytest.mark.parametrize("name", OC.PART)
def test_part_time_steps(built, name, prec):
    """Three steps (G 4, L 2) under FS3D_SWEEP_AUTO from the seeded state; the closed twin walks beside it and is printed."""
    dtype, f64_part, P = PREC[prec]
    ref = OC.steps_reference(name, dtype)
    s, tw = make(name, dtype, capi.SWEEP_AUTO, f64_part=f64_part), make(name, dtype, capi.SWEEP_AUTO, f64_part=f64_part, closed=True)
    OC.seed_all(name, s=s); OC.seed_all(name, s=tw, closed=True)
    for step in range(3):
        s.UpdateBoundaries(); tw.UpdateBoundaries()
        e = s.TimeStep(DT, 4, 2, True); tw.TimeStep(DT, 4, 2, True)
        assert e == pytest.approx(ref[step].err, rel=1e-4 if prec == "f32" else P64.TOL_DIV_ERR)
        o = part_step_check(s, name, prec, step, "%s %s: cur after step %d" % (name, prec, step))
        c = part_step_check(tw, name, prec, step, "", closed=True, check=False)
        print("DIST steps %s %s step %d: velocity %.2e T %.2e (closed twin %.2e %.2e); the oracle's fp32 vs fp64: %.2e (closed twin %.2e)" % (
            prec, name, step, o[0], o[1], c[0], c[1], oracle_fp32_deviation(name, step), oracle_fp32_deviation(name, step, True)))
    k = s.last_sweep_kernels()
    if OC.grid(name).dimz % 4 == 0:
        assert k == {"X": "part", "Y": "part", "Z": "part"}, k
    else:                                                # no whole 16-byte pieces for the Z kernels: the thread-per-line walk
        assert (k["X"], k["Y"], k["Z"]) == ("part", "part", "line"), k
    s.close(); tw.close()


# ---- d. x-slabs -------------------------------------------------------------------------------------------------------------

SLABS = [("x_obstacle_then_open", 2), ("x_obstacle_then_open", 4), ("x_through", 3), ("z_hi", 2)]


def slab_steps(name, nranks, kernel, xsolve):
    """Three steps (G 4, L 2) from the seeded state on nranks x-slabs: cur, next, the X kernel names, stale_in_cells per slab."""
    g = OC.grid(name)
    grp = capi.LocalGroup(g, capi.fluid_params(np.float32, *OC.PARAMS), nranks, np.float32)

    def work(r, sv):
        sv.set_option(capi.OPT_SWEEP_KERNEL, kernel)
        if xsolve is not None:
            sv.set_option(capi.OPT_XSOLVE, xsolve)
        OC.seed_all(name, s=sv, x=slice(*slab_range(g.dimx, r, nranks)))
        for i in range(3):
            sv.UpdateBoundaries(); sv.TimeStep(DT, 4, 2, True)
        return sv.download_layer(capi.LAYER_CUR), sv.download_layer(capi.LAYER_NEXT), sv.last_sweep_kernels()["X"], sv.geometry_info()["stale_in_cells"]
    try:
        res = grp.run(work)
    finally:
        grp.close()
    cat = lambda k: [np.concatenate([r[k][v] for r in res], axis=0) for v in range(4)]
    return cat(0), cat(1), [r[2] for r in res], [r[3] for r in res]


@pytest.mark.parametrize("name,nranks", SLABS)
def test_slabs_exact_kernels(built, name, nranks):
    """x_obstacle_then_open on four 7-plane slabs: one holds the END cell and the start of the tail, the last nothing but tail;
    x_through: no slab has a segment on those lines.  The pipelined X solve carries the recurrence from rank to rank."""
    want = OC.steps_reference(name, np.float32)[2]
    cur, nxt, names, stale = slab_steps(name, nranks, capi.SWEEP_EXACT, capi.XSOLVE_PIPELINED)
    print("%s on %d ranks: %s, stale cells per slab %s" % (name, nranks, names, stale))
    assert all("pipelined-ranks" in k for k in names), names
    assert sum(stale) == host_stale_count(name)
    one = make(name, np.float32, capi.SWEEP_EXACT)
    OC.seed_all(name, s=one)
    for i in range(3):
        one.UpdateBoundaries(); one.TimeStep(DT, 4, 2, True)
    assert_equal(cur, one.download_layer(capi.LAYER_CUR), "%s %d ranks vs one context: cur" % (name, nranks))
    assert_equal(nxt, one.download_layer(capi.LAYER_NEXT), "%s %d ranks vs one context: next" % (name, nranks))
    one.close()
    assert_equal(cur, want.cur, "%s %d ranks vs the oracle: cur" % (name, nranks))
    assert_equal(nxt, want.next, "%s %d ranks vs the oracle: next" % (name, nranks))


@pytest.mark.parametrize("name,nranks", SLABS)
def test_slabs_default_x_solve(built, name, nranks):
    """FS3D_SWEEP_AUTO: partition kernels for Y and Z, the reduced-interface X solve, held to the bound of the single context."""
    cur, _, names, stale = slab_steps(name, nranks, capi.SWEEP_AUTO, None)
    assert all("reduced-interface" in k for k in names), names
    assert sum(stale) == host_stale_count(name)
    dist = part_step_check(cur, name, "f32", 2, "%s on %d slabs: cur after 3 steps" % (name, nranks))
    print("DIST slabs %s %d ranks %s: velocity %.2e T %.2e" % (name, nranks, names[0], dist[0], dist[1]))


# ---- e. a geometry that opens and closes between steps ----------------------------------------------------------------------

SEQUENCE = [("z_hi", False), ("y_hi", False), ("z_hi", True)]         # after a step on the closed box; (case, closed twin)
G_OPEN = 3                                                            # G >= 2: the dropped X store is live on the closed box


def open_and_close(kernel, dev):
    """One context walks closed box -> z_hi -> y_hi -> closed box, a step on each.  After every update: the tables, then the step,
    equal a fresh context's on that geometry with the same four layers; on the exact kernels also the oracle's, which is driven
    through the same geometries.  The fused step's stale_in_cells guard changes value three times in this context's life."""
    dtype = np.float32
    table_keys = capi.Solver.GEOMETRY_INFO[:13]
    exact = kernel == capi.SWEEP_EXACT
    a = make("z_hi", dtype, kernel, closed=True)
    o = OC.oracle("z_hi", dtype, closed=True)
    OC.seed_all("z_hi", s=a, o=o)

    def step(s):
        s.UpdateBoundaries()
        return s.TimeStep(DT, G_OPEN, 2, True)
    step(a)
    o.update_boundaries(); o.time_step(DT, G_OPEN, 2, True)
    assert a.geometry_info()["stale_in_cells"] == 0
    for name, closed in SEQUENCE:
        g = OC.grid(name, closed)
        arrs = [np.ascontiguousarray(x, np.uint8) for x in (g.type, g.bc_vel, g.bc_temp)] + [np.ascontiguousarray(x, dtype) for x in (g.vx, g.vy, g.vz, g.T)]
        if dev:
            import torch
            ten = [torch.from_numpy(x).cuda() for x in arrs]
            torch.cuda.synchronize()
            nseg = a.update_nodes_dev(*ten)
        else:
            nseg = a.update_nodes(g)
        o.set_nodes(g)
        b = make(name, dtype, kernel, closed=closed)
        for l in OC.LAYERS:
            b.upload_layer(l, a.download_layer(l))
        ia, ib = a.geometry_info(), b.geometry_info()
        assert [ia[k] for k in table_keys] == [ib[k] for k in table_keys], (ia, ib)
        assert nseg == b.num_segments == [o.num_segments(d) for d in range(3)]
        assert ia["stale_in_cells"] == (0 if closed else host_stale_count(name))
        ea, eb = step(a), step(b)
        o.update_boundaries()
        rc, eo = o.time_step(DT, G_OPEN, 2, True)
        assert ea == eb and rc == 0
        for layer in (capi.LAYER_CUR, capi.LAYER_NEXT):
            A, B = a.download_layer(layer), b.download_layer(layer)
            for v in range(4):
                assert np.array_equal(bits(A[v]), bits(B[v])), "%s, layer %d field %d: update and fresh context differ in %d cells" % (
                    name, layer, v, int((bits(A[v]) != bits(B[v])).sum()))
            if exact:
                assert_equal(A, o.get_layer_fields(layer), "%s%s, layer %d vs the oracle" % (name, " (closed)" if closed else "", layer))
        if exact:
            assert ea == pytest.approx(eo, rel=1e-12)
        assert a.last_sweep_kernels() == b.last_sweep_kernels()
        b.close()
    k = a.last_sweep_kernels()
    assert set(k.values()) == ({"pipe"} if exact else {"part"}), k
    a.close(); o.close()


@pytest.mark.parametrize("kernel", [capi.SWEEP_EXACT, capi.SWEEP_AUTO])
def test_geometry_opens_and_closes(built, kernel):
    open_and_close(kernel, dev=False)


@pytest.mark.parametrize("kernel", [capi.SWEEP_EXACT, capi.SWEEP_AUTO])
def test_geometry_opens_and_closes_from_device_arrays(built, kernel):
    """update_nodes_dev takes torch tensors: a fresh process in which torch opens the GPU first, as tests/test_gpu_moving.py."""
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "dev", str(kernel)], capture_output=True, text=True, timeout=600)
    print(r.stdout[-5000:], r.stderr[-5000:])
    assert r.returncode == 0 and "__OPEN_CLOSE_OK__" in r.stdout, r.stderr[-3000:]


# ---- f. time_step_async -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kernel", [capi.SWEEP_AUTO, capi.SWEEP_EXACT])
def test_async_step_on_whole_stale_lines(built, kernel):
    """fs3d_time_step_async == UpdateBoundaries + TimeStep bit for bit on z_through (G 3: the X store guard is live); the exact
    kernels also equal the oracle."""
    name, G, L = "z_through", 3, 2
    a, b = make(name, np.float32, kernel), make(name, np.float32, kernel)
    OC.seed_all(name, s=a); OC.seed_all(name, s=b)
    for i in range(3):
        a.UpdateBoundaries(); a.TimeStep(DT, G, L, i == 1)
        b.time_step_async(DT, G, L)
    b.synchronize()
    want = OC.steps_reference(name, np.float32, G, L)[2]
    for layer, ref in ((capi.LAYER_CUR, want.cur), (capi.LAYER_NEXT, want.next)):
        A, B = a.download_layer(layer), b.download_layer(layer)
        for x, y in zip(A, B):
            assert np.array_equal(bits(x), bits(y))
        if kernel == capi.SWEEP_EXACT:
            assert_equal(B, ref, "z_through, layer %d vs the oracle" % layer)
    assert a.eval_div_error(capi.LAYER_CUR) == b.eval_div_error(capi.LAYER_CUR)
    a.close(); b.close()


if __name__ == "__main__":
    import torch
    torch.cuda.init()                    # before the library opens the device
    if sys.argv[1] == "dev":
        open_and_close(int(sys.argv[2]), dev=True)
        print("__OPEN_CLOSE_OK__")
