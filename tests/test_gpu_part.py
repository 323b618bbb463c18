"""GPU parity tests of the partition (reduced-interface) sweep kernels -- FS3D_SWEEP_PART, what FS3D_SWEEP_AUTO runs
in fp32 (csrc/kernels_part.hip) -- against the CPU oracle on the same inputs, through the C ABI.

These kernels solve the reference's equations with the chunks of a line eliminated at the same time; the algebra is
exact, the rounding differs from the sequential Thomas recurrence (Common/Algorithms.h:21-38).  Stated tolerances
(fp32, rel-L2 = ||hip - oracle|| / ||oracle|| over the whole grid):
    one sweep (+ fused merge)                    every field           <= 5e-7   (measured 1e-8 .. 3e-7)
    time steps (G = 4, L = 2), velocity as a vector field and T, grids up to 64^3 .. 70x40x36:
        <= 10 steps                                                   <= 1e-6   (measured 2.4e-7 .. 7.3e-7)
        100 steps of the shipped 64^3 example                         <= 1e-6   (measured 3.9e-7; the reference's own fp32
                                                                                 build differs from its fp64 build by
                                                                                 2.9e-7 .. 2.6e-6 per component there)
    the divergence error printed every 10th step                      <= 1e-4 relative
    128^3 and 256^3 (h = 1/127, 1/255: every rounding of T ~ 1 enters the momentum rows through dT/ds, i.e. times 1/2h,
    and the flow starts from rest): the yardstick is the fp64 solution -- the partition kernels must not deviate from it by
    more than 1.5 x what the reference's own sequential fp32 arithmetic (the bit-exact kernels) deviates, and <= 5e-6.
The small components v, w (|v| << |u| in these channel flows) are also held to 1e-5 of THEIR OWN norm.
"""
import os

import numpy as np
import pytest

from cmc_fluid_solver_amd import capi, grids

pytestmark = pytest.mark.gpu

DT = 0.1
PARAMS = (200.0, 0.72, 1.4)
TOL_SWEEP = 5e-7
TOL_STEPS = 1e-6
TOL_100 = 1e-6
TOL_SMALL_COMPONENT = 1e-5
INP = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "inputs")


def _oracle():
    from oracle import oracle as O
    return O


def rel(a, b):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def vec_rel(A, B):
    """velocity as a vector field: ||(du, dv, dw)|| / ||(u, v, w)||"""
    num = sum(np.linalg.norm(np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2 for a, b in zip(A[:3], B[:3]))
    den = sum(np.linalg.norm(np.asarray(b, np.float64)) ** 2 for b in B[:3])
    return float(np.sqrt(num / max(den, 1e-300)))


def make_pair(g, kernel=capi.SWEEP_PART, fuse=1):
    O = _oracle()
    params = capi.fluid_params(np.float32, *PARAMS)
    s = capi.Solver(g, params, np.float32)
    s.set_option(capi.OPT_SWEEP_KERNEL, kernel)
    s.set_option(capi.OPT_FUSE_MERGE, fuse)
    return s, O.Oracle(g, params, np.float32)


def seed_state(s, o, g, seed=1234, scale=None):
    O = _oracle()
    base = [np.ascontiguousarray(a, np.float32) for a in (g.vx, g.vy, g.vz, g.T)]
    cur, tmp = grids.perturb(base, seed=seed), grids.perturb(base, seed=seed + 1)
    s.upload_layer(capi.LAYER_CUR, cur); s.upload_layer(capi.LAYER_TEMP, tmp)
    for v in range(4):
        o.set_field(O.L_CUR, v, cur[v]); o.set_field(O.L_TEMP, v, tmp[v])


def assert_fields_close(s, o, layer_s, layer_o, tol, what):
    A, B = s.download_layer(layer_s), o.get_layer_fields(layer_o)
    for v, (a, b) in enumerate(zip(A, B)):
        assert np.isfinite(a).all(), "%s: field %d has non-finite values" % (what, v)
        r = rel(a, b)
        assert r <= tol, "%s: field %d rel-L2 %.2e > %.1e" % (what, v, r, tol)


def assert_step_close(s, o, tol, what):
    O = _oracle()
    A, B = s.download_layer(capi.LAYER_CUR), o.get_layer_fields(O.L_CUR)
    rv, rt = vec_rel(A, B), rel(A[3], B[3])
    print("%s: velocity rel-L2 %.2e, T %.2e, components %s" % (what, rv, rt, ["%.1e" % rel(a, b) for a, b in zip(A[:3], B[:3])]))
    assert rv <= tol and rt <= tol, "%s: velocity rel-L2 %.2e, T rel-L2 %.2e > %.1e" % (what, rv, rt, tol)
    for v in range(3):
        r = rel(A[v], B[v])
        assert r <= TOL_SMALL_COMPONENT, "%s: component %d rel-L2 %.2e of its own norm" % (what, v, r)


GRIDS = {
    "box_20x24x28": lambda: grids.box(20, 24, 28, h=0.04),
    "obstacle_28x24x32": lambda: grids.box_with_obstacle(28, 24, 32, h=0.03),
    "obstacle_70x40x36": lambda: grids.box_with_obstacle(70, 40, 36, h=0.02),       # lanes past the lane axis, partial chunks
    "box_130x100x64": lambda: grids.box(130, 100, 64, h=0.01),
    "obstacle_256x16x48": lambda: grids.box_with_obstacle(256, 16, 48, h=0.004),     # full-length X lines
    "obstacle_12x256x40": lambda: grids.box_with_obstacle(12, 256, 40, h=0.004),     # full-length Y lines
    "obstacle_10x20x256": lambda: grids.box_with_obstacle(10, 20, 256, h=0.004),     # full-length Z lines (64 lanes per line)
    "obstacle_9x7x128": lambda: grids.box_with_obstacle(9, 7, 128, h=0.01),          # two lines per wave-wide access, odd line count
    "obstacle_6x9x512": lambda: grids.box_with_obstacle(6, 9, 512, h=0.002),         # Z lines held by a pair of waves, full length
    "obstacle_8x10x388": lambda: grids.box_with_obstacle(8, 10, 388, h=0.003),       # pair of waves, the upper one partly past the line
    "box_7x6x260": lambda: grids.box(7, 6, 260, h=0.004),                            # pair of waves, one piece in the upper one
}


@pytest.mark.parametrize("gname", list(GRIDS))
@pytest.mark.parametrize("d", [0, 1, 2])
def test_single_sweep_within_tolerance(built, d, gname):
    """SolveSegments of one direction (AdiSolver3D.cpp:593-603): `next` of every segment cell, nothing else written."""
    O = _oracle()
    g = GRIDS[gname]()
    s, o = make_pair(g)
    assert s.num_segments == [o.num_segments(k) for k in range(3)]
    seed_state(s, o, g)
    sentinel = [np.full(g.shape, 7.25, np.float32) for _ in range(4)]          # cells off the segments must keep it
    s.upload_layer(capi.LAYER_NEXT, sentinel)
    for v in range(4):
        o.set_field(O.L_NEXT, v, sentinel[v])
    s.sweep(d, DT, capi.LAYER_CUR, capi.LAYER_TEMP, capi.LAYER_NEXT, merge=False)
    assert s.last_sweep_kernels()["XYZ"[d]] == "part"
    o.sweep(d, DT, O.L_CUR, O.L_TEMP, O.L_NEXT)
    assert_fields_close(s, o, capi.LAYER_NEXT, O.L_NEXT, TOL_SWEEP, "next after sweep %d" % d)
    for a, b in zip(s.download_layer(capi.LAYER_NEXT), o.get_layer_fields(O.L_NEXT)):
        assert np.array_equal(a == 7.25, b == 7.25), "the set of written cells differs from the reference's"
    for a, b in zip(s.download_layer(capi.LAYER_TEMP), o.get_layer_fields(O.L_TEMP)):
        assert np.array_equal(a, b), "temp must be untouched by a sweep without merge"


@pytest.mark.parametrize("fuse", [0, 1])
@pytest.mark.parametrize("d", [0, 1, 2])
def test_sweep_with_merge_within_tolerance(built, d, fuse):
    """Sweep + next->MergeLayerTo(temp, NODE_IN) (AdiSolver3D.cpp:651) twice: the second sweep reads the merged temp."""
    O = _oracle()
    g = GRIDS["obstacle_70x40x36"]()
    s, o = make_pair(g, fuse=fuse)
    seed_state(s, o, g)
    for _ in range(2):
        s.sweep(d, DT, capi.LAYER_CUR, capi.LAYER_TEMP, capi.LAYER_NEXT, merge=True)
        o.sweep(d, DT, O.L_CUR, O.L_TEMP, O.L_NEXT); o.merge(O.L_NEXT, O.L_TEMP)
    # The second sweep reads a merged temp that differs from the oracle's in the last bit of T ~ 1; the momentum row of the
    # sweep direction carries -v_T dT/ds: 6e-8 / (2h) against velocities of 0.05 in this seeded state -> a few 1e-6 of that
    # component (the oracle's own rounding noise is amplified the same way); the other fields stay at TOL_SWEEP.
    A, B = s.download_layer(capi.LAYER_NEXT), o.get_layer_fields(O.L_NEXT)
    for v in range(4):
        assert rel(A[v], B[v]) <= (5e-6 if v == d else TOL_SWEEP), "next: field %d rel-L2 %.2e" % (v, rel(A[v], B[v]))
    assert_fields_close(s, o, capi.LAYER_TEMP, O.L_TEMP, 5e-6, "merged temp")
    # cells that are not NODE_IN are copied, not merged: bit-equal
    notin = g.type != grids.NODE_IN
    for a, b in zip(s.download_layer(capi.LAYER_TEMP), o.get_layer_fields(O.L_TEMP)):
        assert np.array_equal(a[notin], b[notin])


@pytest.mark.parametrize("gname", ["box_20x24x28", "obstacle_28x24x32", "obstacle_70x40x36"])
@pytest.mark.parametrize("fuse", [0, 1])
def test_time_steps_within_tolerance(built, gname, fuse):
    """UpdateBoundaries + TimeStep (AdiSolver3D.cpp:286-391), 3 steps, G = 4, L = 2, from the node state."""
    O = _oracle()
    g = GRIDS[gname]()
    s, o = make_pair(g, capi.SWEEP_AUTO, fuse)
    for step in range(3):
        s.UpdateBoundaries(); o.update_boundaries()
        e = s.TimeStep(DT, 4, 2, True)
        rc, eo = o.time_step(DT, 4, 2, True)
        assert rc == 0 and e == pytest.approx(eo, rel=1e-4)
        assert_step_close(s, o, TOL_STEPS, "cur after step %d" % step)
    assert s.last_sweep_kernels() == {"X": "part", "Y": "part", "Z": "part"}     # AUTO = the partition kernels in fp32


@pytest.mark.parametrize("GL", [(1, 1), (2, 1), (1, 3), (3, 2)])
def test_other_iteration_counts(built, GL):
    O = _oracle()
    g = GRIDS["obstacle_28x24x32"]()
    s, o = make_pair(g)
    for step in range(2):
        s.UpdateBoundaries(); o.update_boundaries()
        e = s.TimeStep(DT, GL[0], GL[1], True); rc, eo = o.time_step(DT, GL[0], GL[1], True)
        assert rc == 0 and e == pytest.approx(eo, rel=1e-4)
    assert_step_close(s, o, TOL_STEPS, "cur")


def test_dims_outside_the_partition_kernels(built):
    """FS3D_SWEEP_PART never falls back silently; FS3D_SWEEP_AUTO does fall back (to the bit-exact kernels) and says so."""
    O = _oracle()
    g = grids.box(12, 14, 70, h=0.02)          # 70-cell Z lines: not a whole number of 16-byte pieces
    s, o = make_pair(g, capi.SWEEP_PART)
    s.sweep(0, DT, capi.LAYER_CUR, capi.LAYER_TEMP, capi.LAYER_NEXT)
    with pytest.raises(capi.Fs3dError) as ei:
        s.sweep(2, DT, capi.LAYER_CUR, capi.LAYER_TEMP, capi.LAYER_NEXT)
    assert ei.value.status == capi.ERR_UNSUPPORTED
    s2, o2 = make_pair(g, capi.SWEEP_AUTO)
    seed_state(s2, o2, g)
    s2.sweep(2, DT, capi.LAYER_CUR, capi.LAYER_TEMP, capi.LAYER_NEXT)
    o2.sweep(2, DT, O.L_CUR, O.L_TEMP, O.L_NEXT)
    assert s2.last_sweep_kernels()["Z"] in ("pipe", "line")
    for a, b in zip(s2.download_layer(capi.LAYER_NEXT), o2.get_layer_fields(O.L_NEXT)):
        assert np.array_equal(a, b)
    # fp64: the partition kernels are fp32 only; AUTO runs the exact kernels and stays bit-equal
    params = capi.fluid_params(np.float64, *PARAMS)
    g3 = GRIDS["obstacle_28x24x32"]()
    s3 = capi.Solver(g3, params, np.float64)
    o3 = O.Oracle(g3, params, np.float64)
    s3.UpdateBoundaries(); o3.update_boundaries()
    s3.TimeStep(DT, 4, 2, True); o3.time_step(DT, 4, 2, True)
    assert set(s3.last_sweep_kernels().values()) == {"pipe"}
    for a, b in zip(s3.download_layer(capi.LAYER_CUR), o3.get_layer_fields(O.L_CUR)):
        assert np.array_equal(a, b)
    s3.set_option(capi.OPT_SWEEP_KERNEL, capi.SWEEP_PART)
    with pytest.raises(capi.Fs3dError):
        s3.sweep(0, DT, capi.LAYER_CUR, capi.LAYER_TEMP, capi.LAYER_NEXT)


def test_dead_lines_inside_the_fluid(built):
    """Whole grid lines with no segment cell and no NODE_IN cell (solid bars through the box) run along as INTERIOR rows
    in the kernels; whatever they produce must stay in their lanes -- also with huge values inside the bars."""
    O = _oracle()
    g = grids.box(40, 36, 68, h=0.02)
    bars = np.zeros(g.shape, bool)
    bars[:, 10:13, 20:23] = True; bars[15:18, :, 40:43] = True; bars[25:28, 20:23, :] = True
    grids._set_bound(g, bars, grids.BC_NOSLIP, grids.BC_FREE, (0.0, 0.0, 0.0), 1.0)
    for big in (False, True):
        s, o = make_pair(g)
        base = [np.ascontiguousarray(a, np.float32) for a in (g.vx, g.vy, g.vz, g.T)]
        cur, tmp = grids.perturb(base, seed=5), grids.perturb(base, seed=6)
        if big:
            inner = np.zeros(g.shape, bool)
            inner[:, 11, 21] = True; inner[16, :, 41] = True; inner[26, 21, :] = True
            for f in cur[:3] + tmp[:3]:
                f[inner] = 1e8
        s.upload_layer(capi.LAYER_CUR, cur); s.upload_layer(capi.LAYER_TEMP, tmp)
        for v in range(4):
            o.set_field(O.L_CUR, v, cur[v]); o.set_field(O.L_TEMP, v, tmp[v])
        for d in range(3):
            s.sweep(d, DT, capi.LAYER_CUR, capi.LAYER_TEMP, capi.LAYER_NEXT, merge=True)
            o.sweep(d, DT, O.L_CUR, O.L_TEMP, O.L_NEXT); o.merge(O.L_NEXT, O.L_TEMP)
            A, B = s.download_layer(capi.LAYER_NEXT), o.get_layer_fields(O.L_NEXT)
            fluid = g.type == grids.NODE_IN
            for v in range(4):
                assert np.isfinite(A[v]).all()
                # sweeps in sequence on a seeded state: the sweep-direction component sees the last-bit differences of the
                # merged T through dT/ds (see test_sweep_with_merge_within_tolerance)
                assert rel(A[v][fluid], B[v][fluid]) <= (2e-5 if big else (5e-6 if v == d else TOL_SWEEP)), "dir %d field %d" % (d, v)
        s.close(); o.close()


def test_shipped_example_100_steps(built):
    """BASELINE configs[2]-sized parity case: the reference's shipped 64^3 box_pipe example (data + config unchanged), all
    100 steps.  Drift against the fp32 oracle stays inside the reference's own fp32-vs-fp64 drift; the err
    trace starts at 1.25e-5 and ends at 2.3e-5 as the reference binary printed."""
    from cmc_fluid_solver_amd import shape2d
    O = _oracle()
    nodes, cfg, dt = shape2d.load_case(os.path.join(INP, "box_pipe_2D_data.txt"), os.path.join(INP, "box_pipe_2D_config.txt"))
    params = capi.fluid_params(np.float32, cfg.Re, cfg.Pr, cfg.lam)
    s = capi.Solver(nodes, params, np.float32)
    o = O.Oracle(nodes, params, np.float32)
    errs = []
    for i in range(100):
        ce = (i % 10 == 0) or i == 99
        s.UpdateBoundaries(); o.update_boundaries()
        e = s.TimeStep(dt, cfg.num_global, cfg.num_local, ce)
        rc, eo = o.time_step(dt, cfg.num_global, cfg.num_local, ce)
        assert rc == 0
        if ce:
            assert e == pytest.approx(eo, rel=1e-4)
        errs.append(e)
        if i == 9:
            assert_step_close(s, o, TOL_STEPS, "after 10 steps")
    assert s.last_sweep_kernels() == {"X": "part", "Y": "part", "Z": "part"}
    A, B = s.download_layer(capi.LAYER_CUR), o.get_layer_fields(O.L_CUR)
    rv, rt = vec_rel(A, B), rel(A[3], B[3])
    print("64^3 x 100 steps: velocity rel-L2 %.2e, T %.2e, components %s" % (rv, rt, ["%.1e" % rel(a, b) for a, b in zip(A[:3], B[:3])]))
    assert rv <= TOL_100 and rt <= TOL_100
    assert round(errs[0] * 1e5, 2) == 1.25 and round(errs[-1] * 1e5, 1) == 2.3


def test_masked_bottom_geometry(built):
    """BASELINE configs[4] in small: non_uniform_pipe (depth_var 0.2), 5 steps, against the oracle."""
    from cmc_fluid_solver_amd import shape2d
    O = _oracle()
    nodes, cfg, dt = shape2d.load_case(os.path.join(INP, "non_uniform_pipe_2D_data.txt"), os.path.join(INP, "non_uniform_pipe_2D_config.txt"))
    params = capi.fluid_params(np.float32, cfg.Re, cfg.Pr, cfg.lam)
    s = capi.Solver(nodes, params, np.float32)
    o = O.Oracle(nodes, params, np.float32)
    for i in range(5):
        s.UpdateBoundaries(); o.update_boundaries()
        e = s.TimeStep(dt, cfg.num_global, cfg.num_local, True)
        rc, eo = o.time_step(dt, cfg.num_global, cfg.num_local, True)
        assert rc == 0 and e == pytest.approx(eo, rel=1e-4)
    assert "part" in s.last_sweep_kernels().values()
    assert_step_close(s, o, TOL_STEPS, "cur after 5 steps")


def _yardstick(A, E32, F64, what):
    """deviation from the fp64 solution: partition kernels (A) vs the reference's sequential fp32 arithmetic (E32)"""
    ep, er = vec_rel(A, F64), vec_rel(E32, F64)
    tp, tr = rel(A[3], F64[3]), rel(E32[3], F64[3])
    print("%s: velocity rel-L2 vs fp64: partition %.2e, sequential fp32 %.2e; T: %.2e, %.2e; partition vs sequential fp32: %.2e / %.2e" % (
        what, ep, er, tp, tr, vec_rel(A, E32), rel(A[3], E32[3])))
    assert ep <= 1.5 * er + 1e-7 and tp <= 1.5 * tr + 1e-7, "deviates from the fp64 solution by more than 1.5 x the reference's fp32 arithmetic"
    assert ep <= 5e-6 and tp <= 5e-6


def test_oracle_spot_check_128(built):
    """One step of the 128^3 box (BASELINE configs[1]'s grid) against the CPU oracle in fp32 and fp64."""
    O = _oracle()
    g = grids.box(128, h=1.0 / 127)
    s, o = make_pair(g, capi.SWEEP_AUTO)
    o64 = O.Oracle(g, capi.fluid_params(np.float64, *PARAMS), np.float64)
    s.UpdateBoundaries(); o.update_boundaries(); o64.update_boundaries()
    e = s.TimeStep(DT, 4, 2, True); rc, eo = o.time_step(DT, 4, 2, True); o64.time_step(DT, 4, 2, True)
    assert rc == 0 and e == pytest.approx(eo, rel=1e-4)
    _yardstick(s.download_layer(capi.LAYER_CUR), o.get_layer_fields(O.L_CUR), o64.get_layer_fields(O.L_CUR), "128^3 after 1 step")


def _three_solvers(nodes, steps):
    """the partition kernels (fp32), the bit-exact kernels in fp32 and in fp64 (= the CPU oracle's values, test_gpu_parity.py)"""
    out = []
    for dtype, kernel in ((np.float32, capi.SWEEP_AUTO), (np.float32, capi.SWEEP_EXACT), (np.float64, capi.SWEEP_EXACT)):
        s = capi.Solver(nodes, capi.fluid_params(dtype, *PARAMS), dtype)
        s.set_option(capi.OPT_SWEEP_KERNEL, kernel)
        errs = []
        for i in range(steps):
            s.UpdateBoundaries()
            errs.append(s.TimeStep(0.1, 4, 2, True))
        out.append((s.download_layer(capi.LAYER_CUR), errs, s.last_sweep_kernels()))
        s.close()
    return out


def test_full_size_256(built):
    """BASELINE configs[2] (256^3 fp32 box), 3 steps: the partition kernels against the fp64 solution, next to what the
    reference's own sequential fp32 arithmetic deviates from it; the divergence errors; the box's mirror symmetry in y."""
    g = grids.box(256, h=1.0 / 255)
    (A, ea, ka), (B, eb, kb), (C, ec, kc) = _three_solvers(g, 3)
    assert set(ka.values()) == {"part"} and set(kb.values()) == {"pipe"}
    _yardstick(A, B, C, "256^3 box after 3 steps")
    for a, b in zip(ea, eb):
        assert a == pytest.approx(b, rel=1e-4)
    u = A[0].astype(np.float64)
    assert np.abs(u - u[:, ::-1, :]).max() <= 2e-5 * np.abs(u).max()            # y mirror (the partition is not mirror-symmetric in rounding)
    # (r3) ... and directly against the CPU path at this size: the CPU oracle -- bit-equal to the reference's own
    # binary at 256^3 (tests/test_ref_golden.py) -- walks the same 3 steps; the exact kernels must equal it bit for bit, the production
    # kernels stay inside the distance bench.py publishes with the throughput (`parity_check`: 2.9e-6 / 1.7e-6 measured)
    O = _oracle()
    o = O.Oracle(g, capi.fluid_params(np.float32, *PARAMS), np.float32)
    for i in range(3):
        o.update_boundaries(); o.time_step(0.1, 4, 2, True)
    E = o.get_layer_fields(O.L_CUR)
    o.close()
    for b, e in zip(B, E):
        assert np.array_equal(b, e), "exact kernels differ from the CPU oracle at 256^3"
    rv, rt = vec_rel(A, E), rel(A[3], E[3])
    print("256^3 box after 3 steps: production kernels vs the CPU oracle: velocity %.2e, T %.2e" % (rv, rt))
    assert rv <= 4.5e-6 and rt <= 2.6e-6


def test_masked_geometry_256(built):
    """BASELINE configs[4] at full size: non_uniform_pipe (depth_var 0.2) at dx 0.0042 -> 256^3 through the loader, 2 steps."""
    from cmc_fluid_solver_amd import shape2d
    nodes, _ = shape2d.load_shape2d(os.path.join(INP, "non_uniform_pipe_2D_data.txt"), float(np.float32(0.0042)), float(np.float32(0.0042)),
                                    float(np.float32(0.0042)), 1.0, depth_var=float(np.float32(0.2)), baseT=1.0, align=True)
    assert nodes.shape == (256, 256, 256)
    (A, ea, ka), (B, eb, kb), (C, ec, kc) = _three_solvers(nodes, 2)
    assert set(ka.values()) == {"part"}
    _yardstick(A, B, C, "256^3 masked geometry after 2 steps")
    for a, b in zip(ea, eb):
        assert a == pytest.approx(b, rel=1e-4)


# ---- cross-slab X sweep, reduced-interface form (all ranks at once, one all-gather per sweep) -----------------------
@pytest.mark.parametrize("nranks", [2, 3, 4, 8])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_slabs_reduced_interface_x_solve(built, nranks, dtype):
    """x-slabs through the in-process group (what the RCCL ranks run, minus the wire): the reduced-interface X solve
    (AdiSolver3D.cu:524-640 replaced: every rank eliminates its slab at once) against ONE context on the same kernels
    otherwise -- single sweeps on a seeded state and three time steps.  Equal to rounding (the interface solve rounds
    differently from the sequential recurrence): the fp64 run shows how close 'rounding' is."""
    O = _oracle()
    g = grids.box_with_obstacle(67, 24, 64, h=0.02)              # uneven slabs, an obstacle across slab boundaries
    params = capi.fluid_params(dtype, *PARAMS)
    base = [np.ascontiguousarray(a, dtype) for a in (g.vx, g.vy, g.vz, g.T)]
    cur, tmp = grids.perturb(base, seed=3), grids.perturb(base, seed=4)
    from cmc_fluid_solver_amd.slab import slab_range

    def single():
        s = capi.Solver(g, params, dtype)
        s.set_option(capi.OPT_SWEEP_KERNEL, capi.SWEEP_EXACT)
        s.upload_layer(capi.LAYER_CUR, cur); s.upload_layer(capi.LAYER_TEMP, tmp)
        s.sweep(0, DT, capi.LAYER_CUR, capi.LAYER_TEMP, capi.LAYER_NEXT, merge=True)
        sw = s.download_layer(capi.LAYER_NEXT), s.download_layer(capi.LAYER_TEMP)
        s.close()
        s = capi.Solver(g, params, dtype)
        s.set_option(capi.OPT_SWEEP_KERNEL, capi.SWEEP_EXACT)
        errs = []
        for i in range(3):
            s.UpdateBoundaries(); errs.append(s.TimeStep(DT, 4, 2, True))
        out = sw, s.download_layer(capi.LAYER_CUR), errs
        s.close()
        return out
    (ref_next, ref_temp), ref_cur, ref_errs = single()

    grp = capi.LocalGroup(g, params, nranks, dtype)

    def work(r, sv):
        x0, x1 = slab_range(g.dimx, r, nranks)
        sv.set_option(capi.OPT_SWEEP_KERNEL, capi.SWEEP_EXACT)          # the slab-local kernels as in the single run ...
        sv.set_option(capi.OPT_XSOLVE, capi.XSOLVE_REDUCED)             # ... only the cross-slab solve differs
        sv.upload_layer(capi.LAYER_CUR, [f[x0:x1] for f in cur]); sv.upload_layer(capi.LAYER_TEMP, [f[x0:x1] for f in tmp])
        sv.sweep(0, DT, capi.LAYER_CUR, capi.LAYER_TEMP, capi.LAYER_NEXT, merge=True)
        ran = sv.last_sweep_kernels()["X"]
        sw = sv.download_layer(capi.LAYER_NEXT), sv.download_layer(capi.LAYER_TEMP)
        return ran, sw
    res = grp.run(work)
    assert all("reduced-interface" in r[0] for r in res)
    tol = 5e-7 if dtype == np.float32 else 2e-15
    for v in range(4):
        nx = np.concatenate([res[r][1][0][v] for r in range(nranks)], axis=0)
        tp = np.concatenate([res[r][1][1][v] for r in range(nranks)], axis=0)
        assert rel(nx, ref_next[v]) <= tol and rel(tp, ref_temp[v]) <= tol, "sweep, field %d: %.2e / %.2e" % (v, rel(nx, ref_next[v]), rel(tp, ref_temp[v]))
    grp.close()

    grp = capi.LocalGroup(g, params, nranks, dtype)

    def steps(r, sv):
        sv.set_option(capi.OPT_SWEEP_KERNEL, capi.SWEEP_EXACT)
        sv.set_option(capi.OPT_XSOLVE, capi.XSOLVE_REDUCED)
        errs = []
        for i in range(3):
            sv.UpdateBoundaries(); errs.append(sv.TimeStep(DT, 4, 2, True))
        return sv.download_layer(capi.LAYER_CUR), errs
    res = grp.run(steps)
    full = [np.concatenate([res[r][0][v] for r in range(nranks)], axis=0) for v in range(4)]
    rv, rt = vec_rel(full, ref_cur), rel(full[3], ref_cur[3])
    print("%d slabs, %s, 3 steps: velocity rel-L2 %.2e, T %.2e vs one context" % (nranks, np.dtype(dtype).name, rv, rt))
    assert rv <= (TOL_STEPS if dtype == np.float32 else 1e-13) and rt <= (TOL_STEPS if dtype == np.float32 else 1e-13)
    for r in range(nranks):
        assert res[r][1][-1] == pytest.approx(ref_errs[-1], rel=1e-4 if dtype == np.float32 else 1e-10)
    grp.close()


@pytest.mark.parametrize("dimx,nranks,onchip", [(64, 2, True), (64, 4, True), (96, 3, True), (128, 2, True), (64, 8, True), (72, 3, True), (64, 3, False), (70, 2, False)])
def test_slab_interface_words_from_the_partition_kernel(built, dimx, nranks, onchip):
    """Slabs of whole 16-plane chunks take their 18 interface words per line from a first pass of the X partition kernel
    (rows and chunk elimination on chip) instead of the thread-per-line walk; other slab heights keep the walk.  One merged
    X sweep on a seeded state and two steps, against ONE context on the same kernels: equal to rounding."""
    from cmc_fluid_solver_amd.slab import slab_range
    g = grids.box_with_obstacle(dimx, 24, 64, h=0.02)
    params = capi.fluid_params(np.float32, *PARAMS)
    base = [np.ascontiguousarray(a, np.float32) for a in (g.vx, g.vy, g.vz, g.T)]
    cur, tmp = grids.perturb(base, seed=5), grids.perturb(base, seed=6)
    s = capi.Solver(g, params, np.float32)
    s.upload_layer(capi.LAYER_CUR, cur); s.upload_layer(capi.LAYER_TEMP, tmp)
    s.sweep(0, DT, capi.LAYER_CUR, capi.LAYER_TEMP, capi.LAYER_NEXT, merge=True)
    ref_next, ref_temp = s.download_layer(capi.LAYER_NEXT), s.download_layer(capi.LAYER_TEMP)
    s.close()
    s = capi.Solver(g, params, np.float32)
    for i in range(2):
        s.UpdateBoundaries(); s.TimeStep(DT, 4, 2, True)
    ref_cur = s.download_layer(capi.LAYER_CUR); s.close()
    grp = capi.LocalGroup(g, params, nranks, np.float32)

    def work(r, sv):
        x0, x1 = slab_range(g.dimx, r, nranks)
        sv.upload_layer(capi.LAYER_CUR, [f[x0:x1] for f in cur]); sv.upload_layer(capi.LAYER_TEMP, [f[x0:x1] for f in tmp])
        sv.sweep(0, DT, capi.LAYER_CUR, capi.LAYER_TEMP, capi.LAYER_NEXT, merge=True)
        return sv.last_sweep_kernels()["X"], sv.download_layer(capi.LAYER_NEXT), sv.download_layer(capi.LAYER_TEMP)
    res = grp.run(work)
    grp.close()
    assert all(("on-chip" in r[0]) == onchip and "reduced-interface" in r[0] for r in res), [r[0] for r in res]
    for v in range(4):
        nx = np.concatenate([r[1][v] for r in res], axis=0); tp = np.concatenate([r[2][v] for r in res], axis=0)
        assert rel(nx, ref_next[v]) <= TOL_SWEEP and rel(tp, ref_temp[v]) <= TOL_SWEEP, "field %d: %.2e / %.2e" % (v, rel(nx, ref_next[v]), rel(tp, ref_temp[v]))
    grp = capi.LocalGroup(g, params, nranks, np.float32)

    def steps(r, sv):
        for i in range(2):
            sv.UpdateBoundaries(); sv.TimeStep(DT, 4, 2, True)
        return sv.download_layer(capi.LAYER_CUR)
    res = grp.run(steps)
    grp.close()
    full = [np.concatenate([r[v] for r in res], axis=0) for v in range(4)]
    assert vec_rel(full, ref_cur) <= TOL_STEPS and rel(full[3], ref_cur[3]) <= TOL_STEPS


@pytest.mark.parametrize("n,nslabs", [(64, 4), (64, 8), (128, 2), (128, 8)])
def test_slabs_default_is_the_reduced_interface_solve(built, n, nslabs):
    """FS3D_SWEEP_AUTO on slabs: partition kernels for Y and Z, the reduced-interface X solve; against one context (AUTO).
    (N slabs of the 128^3 box = the self-check bench.py --gpus N runs before it times anything.)"""
    g = grids.box(n, h=1.0 / (n - 1))
    params = capi.fluid_params(np.float32, *PARAMS)
    s = capi.Solver(g, params, np.float32)
    for i in range(2):
        s.UpdateBoundaries(); s.TimeStep(DT, 4, 2, True)
    ref = s.download_layer(capi.LAYER_CUR); s.close()
    grp = capi.LocalGroup(g, params, nslabs, np.float32)

    def steps(r, sv):
        for i in range(2):
            sv.UpdateBoundaries(); sv.TimeStep(DT, 4, 2, True)
        return sv.download_layer(capi.LAYER_CUR), sv.last_sweep_kernels()
    res = grp.run(steps)
    assert res[0][1]["Y"] == "part" and res[0][1]["Z"] == "part" and "reduced-interface" in res[0][1]["X"]
    full = [np.concatenate([res[r][0][v] for r in range(nslabs)], axis=0) for v in range(4)]
    assert vec_rel(full, ref) <= TOL_STEPS and rel(full[3], ref[3]) <= TOL_STEPS
    grp.close()


@pytest.mark.parametrize("nranks", [2, 4])
def test_halo_planes_beside_the_interior_sweep(built, nranks):
    """FS3D_OPT_OVERLAP: interior planes of a slab's Y / Z sweep run beside the halo exchange (second stream), the two edge
    planes after it.  Same kernels on the same cells: the fields equal the exchange-first order bit for bit; three steps."""
    g = grids.box_with_obstacle(64, 40, 64, h=0.02)
    params = capi.fluid_params(np.float32, *PARAMS)
    out = {}
    for overlap in (1, 0):
        grp = capi.LocalGroup(g, params, nranks, np.float32)

        def steps(r, sv):
            sv.set_option(capi.OPT_OVERLAP, overlap)
            errs = []
            for i in range(3):
                sv.UpdateBoundaries(); errs.append(sv.TimeStep(DT, 4, 2, True))
            return sv.download_layer(capi.LAYER_CUR), errs, sv.last_sweep_kernels()
        res = grp.run(steps)
        assert res[0][2]["Y"] == "part" and res[0][2]["Z"] == "part"
        out[overlap] = [np.concatenate([res[r][0][v] for r in range(nranks)], axis=0) for v in range(4)], res[0][1]
        grp.close()
    for a, b in zip(out[1][0], out[0][0]):
        assert np.array_equal(a, b)
    assert out[1][1] == out[0][1]


def test_results_do_not_depend_on_layout_padding_or_workgroup_schedule(built, tmp_path):
    """Every FS3D_* environment variable the production library reads is a speed knob: field padding / layer skew (fs3d_create) and
    the tiling of the X/Y kernels (FS3D_PART_VARIANT) -- the fields after two steps are bit-identical whatever they are set to (each
    setting in a process of its own: the knobs are read once).  The former kernel-experiment knobs (FS3D_PART_ORDER, _LDSPAD,
    _LATE_SLAB, _ZLG) and the experiment-only chunk size (FS3D_PART_VARIANT=10) were removed from the library: setting them must
    change nothing."""
    import subprocess
    import sys
    code = ("import sys, hashlib, numpy as np\n"
            "from cmc_fluid_solver_amd import capi, grids\n"
            "g = grids.box_with_obstacle(136, 150, 64, h=0.01)\n"
            "s = capi.Solver(g, capi.fluid_params(np.float32, 200.0, 0.72, 1.4), np.float32)\n"
            "for i in range(2):\n"
            "    s.UpdateBoundaries(); s.TimeStep(0.1, 2, 2, True)\n"
            "h = hashlib.sha256()\n"
            "for a in s.download_layer(capi.LAYER_CUR): h.update(np.ascontiguousarray(a).tobytes())\n"
            "print('HASH', h.hexdigest(), s.last_sweep_kernels())\n")
    outs = {}
    for tag, env in (("default", {}), ("no padding", {"FS3D_FIELD_PAD": "0", "FS3D_LAYER_SKEW": "0"}), ("big padding", {"FS3D_FIELD_PAD": "4164", "FS3D_LAYER_SKEW": "66048"}),
                     ("experiment knobs are not read by the product", {"FS3D_PART_ORDER": "6", "FS3D_PART_LDSPAD": "8192", "FS3D_PART_LATE_SLAB": "3", "FS3D_PART_ZLG": "2"}),
                     ("64-line tiles", {"FS3D_PART_VARIANT": "64"}), ("32-line tiles", {"FS3D_PART_VARIANT": "32"}), ("16-line tiles", {"FS3D_PART_VARIANT": "16"}),
                     ("other chunk sizes exist in experiment builds only", {"FS3D_PART_VARIANT": "10"})):
        r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **env), capture_output=True, text=True, timeout=300,
                           cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("HASH")]
        assert line, (tag, r.stdout[-300:], r.stderr[-300:])
        outs[tag] = line[0]
    assert "'X': 'part'" in outs["default"]
    assert len(set(outs.values())) == 1, outs


@pytest.mark.parametrize("nranks", [2, 4, 8])
def test_slab_kernels_of_wide_grids(built, nranks):
    """Slabs of a grid wide enough for the 64-line slab kernels (dimy x dimz/64 >= 512 tiles: what a 256^3 run on 2, 4, 8 GPUs launches:
    128-, 64- and 32-plane slabs): one merged X sweep on a seeded state and one step against ONE context."""
    from cmc_fluid_solver_amd.slab import slab_range
    g = grids.box_with_obstacle(256, 256, 128, h=0.004)
    params = capi.fluid_params(np.float32, *PARAMS)
    base = [np.ascontiguousarray(a, np.float32) for a in (g.vx, g.vy, g.vz, g.T)]
    cur, tmp = grids.perturb(base, seed=7), grids.perturb(base, seed=8)
    s = capi.Solver(g, params, np.float32)
    s.upload_layer(capi.LAYER_CUR, cur); s.upload_layer(capi.LAYER_TEMP, tmp)
    s.sweep(0, DT, capi.LAYER_CUR, capi.LAYER_TEMP, capi.LAYER_NEXT, merge=True)
    ref_next, ref_temp = s.download_layer(capi.LAYER_NEXT), s.download_layer(capi.LAYER_TEMP)
    s.close()
    s = capi.Solver(g, params, np.float32)
    s.UpdateBoundaries(); s.TimeStep(DT, 2, 2, True)
    ref_cur = s.download_layer(capi.LAYER_CUR); s.close()
    grp = capi.LocalGroup(g, params, nranks, np.float32)

    def work(r, sv):
        x0, x1 = slab_range(g.dimx, r, nranks)
        sv.upload_layer(capi.LAYER_CUR, [f[x0:x1] for f in cur]); sv.upload_layer(capi.LAYER_TEMP, [f[x0:x1] for f in tmp])
        sv.sweep(0, DT, capi.LAYER_CUR, capi.LAYER_TEMP, capi.LAYER_NEXT, merge=True)
        return sv.last_sweep_kernels()["X"], sv.download_layer(capi.LAYER_NEXT), sv.download_layer(capi.LAYER_TEMP)
    res = grp.run(work)
    grp.close()
    assert all("on-chip" in r[0] for r in res), [r[0] for r in res]
    for v in range(4):
        nx = np.concatenate([r[1][v] for r in res], axis=0); tp = np.concatenate([r[2][v] for r in res], axis=0)
        assert rel(nx, ref_next[v]) <= TOL_SWEEP and rel(tp, ref_temp[v]) <= TOL_SWEEP, "field %d: %.2e / %.2e" % (v, rel(nx, ref_next[v]), rel(tp, ref_temp[v]))
    grp = capi.LocalGroup(g, params, nranks, np.float32)

    def step(r, sv):
        sv.UpdateBoundaries(); sv.TimeStep(DT, 2, 2, True)
        return sv.download_layer(capi.LAYER_CUR)
    res = grp.run(step)
    grp.close()
    full = [np.concatenate([r[v] for r in res], axis=0) for v in range(4)]
    assert vec_rel(full, ref_cur) <= TOL_STEPS and rel(full[3], ref_cur[3]) <= TOL_STEPS


@pytest.mark.parametrize("kernel", [capi.SWEEP_AUTO, capi.SWEEP_EXACT])
def test_async_step_equals_update_boundaries_plus_time_step(built, kernel):
    """fs3d_time_step_async = UpdateBoundaries + TimeStep enqueued without a host synchronisation (what bench.py times; it imposes
    the boundary values on cur and next in one pass over the list): the same fields, bit for bit, as the two calls."""
    g = grids.box_with_obstacle(70, 40, 36, h=0.02)
    params = capi.fluid_params(np.float32, *PARAMS)
    a = capi.Solver(g, params, np.float32); a.set_option(capi.OPT_SWEEP_KERNEL, kernel)
    b = capi.Solver(g, params, np.float32); b.set_option(capi.OPT_SWEEP_KERNEL, kernel)
    for i in range(4):
        a.UpdateBoundaries(); a.TimeStep(DT, 2, 2, i == 2)
        b.time_step_async(DT, 2, 2)
    b.synchronize()
    for layer in (capi.LAYER_CUR, capi.LAYER_NEXT):
        for x, y in zip(a.download_layer(layer), b.download_layer(layer)):
            assert np.array_equal(x, y)
    ea, _ = a.eval_div_error(capi.LAYER_CUR); eb, _ = b.eval_div_error(capi.LAYER_CUR)
    assert ea == eb
    a.close(); b.close()
