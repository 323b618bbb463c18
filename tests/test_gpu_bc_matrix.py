"""Every boundary-row kind in every sweep direction, on the GPU, through the C ABI: the grids of tests/bc_cases.py (their CPU
conditions: tests/test_bc_cases.py) against the CPU oracle.

A segment's first and last row come from a 4-bit row code (START / END, velocity NOSLIP / FREE, temperature NOSLIP / FREE): 24
codes over the three directions.  A FREE row (b = 2, off-diagonal -1) is the only end row that couples to its neighbour, so the
only one that can couple across a chunk edge of the X/Y partition kernels, a lane edge of the Z kernel or a slab cut; the F and P
grids put END and START rows on both sides of those edges, the S grids on both sides of a slab cut.

    bit-exact kernels (FS3D_SWEEP_EXACT, fp32 and fp64)    equal to the oracle value for value; no tolerance
    partition kernels, fp32                                 rel-L2 <= 5e-7 per field as tests/test_gpu_part.py, and per LINE:
        over the cells the fp64 oracle wrote, S = max |x64| per field, e(K) = max over lines of max |K - x64| / S,
        e(kernel) <= 2 e(oracle32) + 2^-23      (bc_cases.check_lines; the 2 is the numpy model's, tests/test_partition_algebra.py)
    partition kernels, fp64                                 the fp32 bounds x 4 x 2^-29 (the rule of tests/test_gpu_part_f64.py)
    time steps                                              the yardstick of tests/test_gpu_part.py (1.5 x the fp32 oracle's
                                                            deviation from the fp64 oracle + 1e-7, and <= 5e-6)
    x-slabs                                                 the same per-line criterion for the slabs and for one context;
                                                            the pipelined X solve on the exact kernels equals one context bit for bit

Largest e(kernel) / e(oracle32) measured on one MI355X (printed with -s: "RATIO ..."), over next and the merged temp, fused and
unfused alike; e(oracle32) was 4.0e-8 .. 7.3e-7 (slabs: 2.0e-8 .. 2.3e-7):
    fp32 partition kernels, F and P grids      X 1.52   Y 1.12   Z 1.70
    fp32, Z lines on a pair of waves (L-Z)     Z 1.16
    fp32, 64-line X tiles (W-X)                X 1.08
    fp64 partition kernels (of the scaled e)   X 0.35   Y 0.36   Z 0.52
    x-slabs, 2 / 3 / 4 ranks (and one context) X 1.32
Time steps (3, G 4, L 2), velocity against the fp64 oracle: partition 1.25e-6 .. 1.74e-6 beside the sequential fp32 recurrence's
1.23e-6 .. 1.53e-6 (ratio <= 1.14); fp64 partition kernels 1.9e-15 .. 2.6e-15 (bound 7.5e-15).
With the velocity-FREE START coupling taken out of part_coefs (mv.c = 0 on a START row) every test of tests/test_gpu_part.py on
box_20x24x28 and obstacle_28x24x32 still passes; here the sweeps of F-A, F-B, F-D and P-FF fail at 3e-4 .. 1e-3 rel-L2.
"""
import functools

import numpy as np
import pytest

import bc_cases as BC
from cmc_fluid_solver_amd import capi, grids
from cmc_fluid_solver_amd.slab import slab_range
from test_gpu_part import TOL_SWEEP, _yardstick, rel
from test_gpu_part_f64 import SCALE

pytestmark = pytest.mark.gpu

DT = BC.DT
LAYERS = (capi.LAYER_CUR, capi.LAYER_TEMP, capi.LAYER_NEXT)


def make(name, dtype, kernel, fuse=1, f64_part=0):
    s = capi.Solver(BC.grid(name), capi.fluid_params(dtype, *BC.PARAMS), dtype)
    s.set_option(capi.OPT_SWEEP_KERNEL, kernel)
    s.set_option(capi.OPT_FUSE_MERGE, fuse)
    if f64_part:
        s.set_option(capi.OPT_F64_PART, f64_part)
    return s


def seed(s, name, x=slice(None)):
    """the seeded state in cur and temp, the sentinel in next (planes x of the grid)"""
    cur, tmp = BC.seeded(name)
    s.upload_layer(capi.LAYER_CUR, [f[x] for f in cur]); s.upload_layer(capi.LAYER_TEMP, [f[x] for f in tmp])
    s.upload_layer(capi.LAYER_NEXT, [np.full(f[x].shape, BC.SENTINEL, s.dtype) for f in cur])


def assert_equal(A, B, what):
    for v, (a, b) in enumerate(zip(A, B)):
        if not np.array_equal(a, b):
            bad = np.argwhere(a != b)
            raise AssertionError("%s: field %d differs at %d cells, first %s: hip=%r oracle=%r" % (what, v, len(bad), bad[0], a[tuple(bad[0])], b[tuple(bad[0])]))


# ---- bit-exact kernels ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("name", BC.F_GRIDS + BC.P_GRIDS + ["E-line"] + BC.L_GRIDS)
def test_exact_kernels_equal_the_oracle(built, name, dtype):
    """One merged sweep per direction on the seeded state, then 2 time steps (G 4, L 2): next, temp and cur value for value."""
    sweeps, cur, errs, rcs = BC.merged_run_reference(name, dtype)
    assert rcs == [0, 0]
    s = make(name, dtype, capi.SWEEP_EXACT)
    s.set_option(capi.OPT_KEEP_TEMP, 1)
    seed(s, name)
    for d in range(3):
        s.sweep(d, DT, *LAYERS, merge=True)
        nxt, tmp = s.download_layer(capi.LAYER_NEXT), s.download_layer(capi.LAYER_TEMP)
        assert_equal(nxt, sweeps[d][0], "%s: next, dir %d" % (name, d))
        assert_equal(tmp, sweeps[d][1], "%s: temp, dir %d" % (name, d))
        for a, b in zip(nxt, sweeps[d][0]):
            assert np.array_equal(a == BC.SENTINEL, b == BC.SENTINEL), "the set of written cells differs from the reference's"
    k = s.last_sweep_kernels()
    print("%s %s: sweep kernels %s" % (name, np.dtype(dtype).name, k))
    assert all(v.split("-")[0] in ("pipe", "line") for v in k.values()), k       # "-segmented": lines longer than one launch holds
    if name == "E-line":
        assert k["Z"] in ("pipe", "line")
    for step in range(2):
        s.UpdateBoundaries()
        e = s.TimeStep(DT, 4, 2, True)
        assert e == pytest.approx(errs[step], rel=1e-12), "diffError step %d" % step
    assert_equal(s.download_layer(capi.LAYER_CUR), cur, "%s: cur after 2 steps" % name)
    s.close()


# ---- partition kernels: single sweeps -------------------------------------------------------------------------------------

def part_sweeps(name, dtype, fuse, scale, family):
    """One context; per direction of the grid an unmerged sweep (rel-L2, per-line, the written cells, temp untouched) and the same
    sweep with the merge (per-line on next and on the merged temp: the fused merge stores both in the sweep's own pass)."""
    g = BC.grid(name)
    R32, R64 = BC.sweep_reference(name, np.float32), BC.sweep_reference(name, np.float64)
    s = make(name, dtype, capi.SWEEP_PART, fuse, f64_part=int(dtype == np.float64))
    _, tmp0 = BC.seeded(name)
    fluid = g.type == grids.NODE_IN
    worst = {}
    for d in BC.DIRS[name]:
        seed(s, name)
        s.sweep(d, DT, *LAYERS, merge=False)
        assert s.last_sweep_kernels()["XYZ"[d]] == "part"
        A = s.download_layer(capi.LAYER_NEXT)
        ref = R64[d][0] if dtype == np.float64 else R32[d][0]
        for v in range(4):
            assert np.isfinite(A[v]).all(), "field %d has non-finite values" % v
            r = rel(A[v], ref[v])
            assert r <= TOL_SWEEP * scale, "next after sweep %d: field %d rel-L2 %.2e > %.1e" % (d, v, r, TOL_SWEEP * scale)
            assert np.array_equal(A[v] == BC.SENTINEL, ref[v] == BC.SENTINEL), "the set of written cells differs from the reference's"
        for a, b in zip(s.download_layer(capi.LAYER_TEMP), tmp0):
            assert np.array_equal(a, b.astype(dtype)), "temp must be untouched by a sweep without merge"
        written = [x != BC.SENTINEL for x in R64[d][0]]
        ratios = BC.check_lines(A, R32[d][0], R64[d][0], written, d, "%s %s %s fuse %d: next" % (name, family, "XYZ"[d], fuse), scale)
        seed(s, name)
        s.sweep(d, DT, *LAYERS, merge=True)
        A, T = s.download_layer(capi.LAYER_NEXT), s.download_layer(capi.LAYER_TEMP)
        ratios += BC.check_lines(A, R32[d][0], R64[d][0], written, d, "%s %s %s fuse %d: next (merged sweep)" % (name, family, "XYZ"[d], fuse), scale)
        ratios += BC.check_lines(T, R32[d][1], R64[d][1], [fluid] * 4, d, "%s %s %s fuse %d: merged temp" % (name, family, "XYZ"[d], fuse), scale)
        for v in range(4):                      # cells that are not NODE_IN are left as they were
            assert np.array_equal(T[v][~fluid], tmp0[v][~fluid].astype(dtype))
        worst["XYZ"[d]] = max(ratios)
    print("RATIO %s %s fuse %d: %s" % (family, name, fuse, {k: "%.2f" % v for k, v in worst.items()}))
    s.close()


@pytest.mark.parametrize("fuse", [0, 1])
@pytest.mark.parametrize("name", BC.F_GRIDS + BC.P_GRIDS + BC.L_GRIDS + ["W-X"])
def test_part_sweeps_fp32(built, name, fuse):
    part_sweeps(name, np.float32, fuse, 1.0, "part-f32")


@pytest.mark.parametrize("name", BC.F_GRIDS + ["P-FF"])
def test_part_sweeps_fp64(built, name):
    """FS3D_OPT_F64_PART = 1 against the fp64 oracle; Z runs two cells per lane, and the F and P positions are even / odd edges too."""
    part_sweeps(name, np.float64, 1, SCALE, "part-f64")


# ---- partition kernels: time steps ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", BC.F_GRIDS + ["P-FF"])
def test_part_time_steps_fp32(built, name):
    """FS3D_SWEEP_AUTO, 3 steps (G 4, L 2) from the node state, the yardstick of tests/test_gpu_part.py as it stands."""
    c32, e32, _ = BC.steps_reference(name, np.float32)
    c64, _, _ = BC.steps_reference(name, np.float64)
    s = make(name, np.float32, capi.SWEEP_AUTO)
    for step in range(3):
        s.UpdateBoundaries()
        e = s.TimeStep(DT, 4, 2, True)
        assert e == pytest.approx(e32[step], rel=1e-4)
        _yardstick(s.download_layer(capi.LAYER_CUR), c32[step], c64[step], "%s after step %d" % (name, step))
    assert s.last_sweep_kernels() == {"X": "part", "Y": "part", "Z": "part"}
    s.close()


@pytest.mark.parametrize("name", BC.F_GRIDS + ["P-FF"])
def test_part_time_steps_fp64(built, name):
    """FS3D_OPT_F64_PART = 1 under AUTO against the fp64 oracle: the bounds tests/test_gpu_part_f64.py holds time steps to."""
    import test_gpu_part_f64 as P64
    c64, e64, _ = BC.steps_reference(name, np.float64)
    s = make(name, np.float64, capi.SWEEP_AUTO, f64_part=1)
    for step in range(3):
        s.UpdateBoundaries()
        e = s.TimeStep(DT, 4, 2, True)
        assert e == pytest.approx(e64[step], rel=P64.TOL_DIV_ERR)
        A = s.download_layer(capi.LAYER_CUR)
        rv, rt = P64.vec_rel(A, c64[step]), rel(A[3], c64[step][3])
        print("%s fp64 step %d: velocity rel-L2 %.2e, T %.2e" % (name, step, rv, rt))
        assert np.isfinite(np.stack(A)).all()
        assert rv <= P64.TOL_STEPS and rt <= P64.TOL_STEPS
        for v in range(3):
            assert rel(A[v], c64[step][v]) <= P64.TOL_SMALL_COMPONENT
    assert s.last_sweep_kernels() == {"X": "part", "Y": "part", "Z": "part"}
    s.close()


# ---- x-slabs ----------------------------------------------------------------------------------------------------------------

def slab_run(name, nranks, kernel, xsolve):
    """One merged X sweep on the seeded state, and 2 steps from the node state on a fresh group: (next, temp, kernel names), cur."""
    g = BC.grid(name)
    params = capi.fluid_params(np.float32, *BC.PARAMS)

    def setup(sv):
        sv.set_option(capi.OPT_SWEEP_KERNEL, kernel)
        if xsolve is not None:
            sv.set_option(capi.OPT_XSOLVE, xsolve)

    def sweep(r, sv):
        setup(sv)
        seed(sv, name, slice(*slab_range(g.dimx, r, nranks)))
        sv.sweep(0, DT, *LAYERS, merge=True)
        return sv.last_sweep_kernels()["X"], sv.download_layer(capi.LAYER_NEXT), sv.download_layer(capi.LAYER_TEMP)

    def steps(r, sv):
        setup(sv)
        for i in range(2):
            sv.UpdateBoundaries(); sv.TimeStep(DT, 4, 2, True)
        return sv.download_layer(capi.LAYER_CUR)
    out = []
    for fn in (sweep, steps):
        grp = capi.LocalGroup(g, params, nranks, np.float32)
        try:
            out.append(grp.run(fn))
        finally:
            grp.close()
    cat = lambda k: [np.concatenate([r[k][v] for r in out[0]], axis=0) for v in range(4)]
    return cat(1), cat(2), [r[0] for r in out[0]], [np.concatenate([r[v] for r in out[1]], axis=0) for v in range(4)]


@functools.lru_cache(maxsize=None)
def single_run(name, kernel):
    """one context: (next, merged temp) of the merged X sweep on the seeded state, cur after 2 steps; computed once, read-only"""
    s = make(name, np.float32, kernel)
    seed(s, name)
    s.sweep(0, DT, *LAYERS, merge=True)
    nxt, tmp = s.download_layer(capi.LAYER_NEXT), s.download_layer(capi.LAYER_TEMP)
    s.close()
    s = make(name, np.float32, kernel)
    for i in range(2):
        s.UpdateBoundaries(); s.TimeStep(DT, 4, 2, True)
    cur = s.download_layer(capi.LAYER_CUR)
    s.close()
    for a in nxt + tmp + cur:
        a.setflags(write=False)
    return nxt, tmp, cur


@pytest.mark.parametrize("nranks", [2, 3, 4])
@pytest.mark.parametrize("name", BC.S_GRIDS)
def test_slabs_reduced_interface(built, name, nranks):
    """AUTO kernels: the reduced-interface X solve with the interface words from the partition kernel (2 ranks: 32-plane slabs,
    4 ranks: whole 16-plane chunks) or from the thread-per-line walk (3 ranks), next to one context on the same kernels.  Both are
    held to the per-line criterion against the fp64 oracle, and after 2 steps to the yardstick of tests/test_gpu_part.py."""
    R32, R64 = BC.sweep_reference(name, np.float32), BC.sweep_reference(name, np.float64)
    written = [x != BC.SENTINEL for x in R64[0][0]]
    nxt, tmp, names, cur = slab_run(name, nranks, capi.SWEEP_AUTO, None)
    print("%s on %d ranks: %s" % (name, nranks, names))
    assert all("reduced-interface" in k and ("on-chip" in k) == (nranks != 3) for k in names), names
    one_next, one_temp, one_cur = single_run(name, capi.SWEEP_AUTO)
    for a, b in zip(nxt, R64[0][0]):
        assert np.array_equal(a == BC.SENTINEL, b == BC.SENTINEL), "the set of written cells differs from the reference's"
    BC.check_lines(one_next, R32[0][0], R64[0][0], written, 0, "%s one context: next" % name)
    BC.check_lines(one_temp, R32[0][1], R64[0][1], written, 0, "%s one context: merged temp" % name)
    ratios = BC.check_lines(nxt, R32[0][0], R64[0][0], written, 0, "%s %d slabs: next" % (name, nranks))
    ratios += BC.check_lines(tmp, R32[0][1], R64[0][1], written, 0, "%s %d slabs: merged temp" % (name, nranks))
    print("RATIO slabs-%d %s: %s" % (nranks, name, {"X": "%.2f" % max(ratios)}))
    c32, c64 = BC.steps_reference(name, np.float32)[0][1], BC.steps_reference(name, np.float64)[0][1]
    _yardstick(one_cur, c32, c64, "%s one context after 2 steps" % name)
    _yardstick(cur, c32, c64, "%s %d slabs after 2 steps" % (name, nranks))


@pytest.mark.parametrize("nranks", [2, 3])
@pytest.mark.parametrize("name", BC.S_GRIDS)
def test_slabs_pipelined_exact_equal_one_context(built, name, nranks):
    """FS3D_XSOLVE_PIPELINED on the bit-exact kernels: the sequential recurrence carried from rank to rank, bit for bit what one
    context computes -- a FREE END row on a slab's first plane reads the plane below the cut."""
    nxt, tmp, names, cur = slab_run(name, nranks, capi.SWEEP_EXACT, capi.XSOLVE_PIPELINED)
    assert all("pipelined-ranks" in k for k in names), names
    one_next, one_temp, one_cur = single_run(name, capi.SWEEP_EXACT)
    assert_equal(nxt, one_next, "%s %d ranks: next" % (name, nranks))
    assert_equal(tmp, one_temp, "%s %d ranks: merged temp" % (name, nranks))
    assert_equal(cur, one_cur, "%s %d ranks: cur after 2 steps" % (name, nranks))
    # and one context is the oracle's
    sweeps, _, _, _ = BC.merged_run_reference(name, np.float32, (0,), 0)
    assert_equal(one_next, sweeps[0][0], "%s one context vs the oracle: next" % name)
    assert_equal(one_temp, sweeps[0][1], "%s one context vs the oracle: merged temp" % name)
