"""The numpy twins of the wall loads: layer_output.wall_loads (FS3D_OPT_OUTPUT_WALL 1 and 2, the `vector` modes WALL_VECTOR and
WALL_SCALARS of the record rule) and TimeStats(wall=True) (FS3D_OPT_TIME_STATS_WALL, FS3D_OPT_OUTPUT_WALL 3 and 4), against
analytic fields, the exposed-face rule against a line walk written straight from fs3d_tables.h line_kinds, the loads against a
per-cell loop, and the driver's refusals of `--time-wall` (decided when the arguments are read: no GPU needed).  The kernels are
held to the twins in test_gpu_wall_loads.py."""
import math
import os
import subprocess

import numpy as np
import pytest

from cmc_fluid_solver_amd import build as B
from cmc_fluid_solver_amd import grids
from cmc_fluid_solver_amd import layer_output as LO
from cmc_fluid_solver_amd import time_stats as TS
from cmc_fluid_solver_amd.grids import BC_FREE, NODE_BOUND, NODE_IN, NODE_OUT, NODE_VALVE

HERE = os.path.dirname(os.path.abspath(__file__))
INPUTS = os.path.join(HERE, "golden", "inputs")
DTYPES = [np.float32, np.float64]
POW2 = (0.25, 0.125, 0.5)
SKIP, INTERIOR, START, END = 0, 1, 2, 3


def fluid_block(dims):
    """Fluid everywhere, NOSLIP boundary conditions, no wall yet: (type, bc_vel, bc_temp)"""
    return np.full(dims, NODE_IN, np.uint8), np.zeros(dims, np.uint8), np.zeros(dims, np.uint8)


def walk_kinds(line):
    """fs3d_tables.h line_kinds on one line of node types: the row kind per cell (START wins on a shared cell), and the INTERIOR cells"""
    n = len(line)
    kinds = [SKIP] * n
    state, start = 0, 0
    for pos in range(n - 1):
        if line[pos + 1] == NODE_IN:
            if state == 0:
                start = pos
            state = 1
        elif state == 1:
            end = pos + 1
            kinds[start] = START
            for s in range(start + 1, end):
                kinds[s] = INTERIOR
            kinds[end] = END
            state = 0
    return kinds


def walked_faces(type):
    """The exposed faces by the definition: six bool arrays x-, x+, y-, y+, z-, z+; and per direction the row kinds"""
    dims = type.shape
    faces = [np.zeros(dims, bool) for _ in range(6)]
    kinds = [np.zeros(dims, np.uint8) for _ in range(3)]
    for d in range(3):
        t = np.moveaxis(type, d, 2)
        kd = np.moveaxis(kinds[d], d, 2)
        fm, fp = np.moveaxis(faces[2 * d], d, 2), np.moveaxis(faces[2 * d + 1], d, 2)
        for a in range(t.shape[0]):
            for b in range(t.shape[1]):
                line = t[a, b]
                k = walk_kinds(line)
                kd[a, b] = k
                for s in range(len(line)):
                    if line[s] not in (NODE_BOUND, NODE_VALVE):
                        continue
                    fm[a, b, s] = s - 1 >= 0 and line[s - 1] == NODE_IN and k[s - 1] == INTERIOR
                    fp[a, b, s] = s + 1 < len(line) and line[s + 1] == NODE_IN and k[s + 1] == INTERIOR
    return faces, kinds


def loop_loads(arrays, fields, spacing, nu, kappa):
    """The rule, cell by cell, in scalar arithmetic of the fields' type: carrier, tau[3], mag, q, area"""
    type, bc_vel, bc_temp = arrays
    R = fields[0].dtype.type
    h = [R(d) for d in spacing]
    A = [h[1] * h[2], h[0] * h[2], h[0] * h[1]]
    nu, kappa = R(nu), R(kappa)
    faces, _ = walked_faces(type)
    out = [np.zeros(type.shape, fields[0].dtype) for _ in range(6)]
    carrier = np.zeros(type.shape, bool)
    for B_ in np.argwhere(np.logical_or.reduce(faces)):
        B_ = tuple(B_)
        area, sums = R(0), [R(0)] * 4
        for n in range(6):
            if not faces[n][B_]:
                continue
            d, s = n // 2, (-1, 1)[n % 2]
            P = tuple(B_[a] + (s if a == d else 0) for a in range(3))
            area = area + A[d]
            for c in range(4):
                if c == d or (bc_temp if c == 3 else bc_vel)[B_] == BC_FREE:
                    continue
                g = (fields[c][P] - fields[c][B_]) / h[d]
                t = (kappa if c == 3 else nu) * g
                sums[c] = sums[c] + A[d] * t
        tau = [sums[c] / area for c in range(3)]
        carrier[B_] = True
        for v, val in enumerate(tau + [np.sqrt((tau[0] * tau[0] + tau[1] * tau[1]) + tau[2] * tau[2]), sums[3] / area, area]):
            assert type_of(val) == fields[0].dtype
            out[v][B_] = val
    return carrier, out


def type_of(v):
    return np.asarray(v).dtype


# ---- analytic fields: power-of-two spacings and values, so fp32 and fp64 agree value for value ----

@pytest.mark.parametrize("dtype", DTYPES)
def test_couette_flow_over_a_plate(dtype):
    dims = (5, 9, 4)
    ty, bv, bt = fluid_block(dims)
    ty[:, 4, :] = NODE_BOUND                                   # a plate at rest with fluid on both sides
    ty[:, 0, :] = ty[:, 8, :] = NODE_BOUND                     # and the two walls that close the lines
    gamma, nu = 8.0, 0.5
    y = (np.arange(9) - 4) * POW2[1]
    U = np.broadcast_to((gamma * np.abs(y))[None, :, None], dims).astype(dtype)      # u = gamma * distance: +x flow on both sides
    zero = np.zeros(dims, dtype)
    w = LO.wall_loads((ty, bv, bt), [U, zero, zero, zero], POW2, nu, 0.25)
    plate = np.zeros(dims, bool)
    plate[:, 4, :] = True
    assert w.carrier[plate].all()
    assert (w.tau[0][plate] == dtype(nu * gamma)).all(), "the same sign on either side of the plate"
    assert not w.tau[1][plate].any() and not w.tau[2][plate].any() and not w.q[plate].any()
    assert (w.mag[plate] == dtype(nu * gamma)).all()
    assert (w.area[plate] == dtype(2 * POW2[0] * POW2[2])).all(), "two y faces"
    # the outer walls feel the flow slowing towards them: tau_x = nu * (u[P] - u[B]) / h < 0
    assert (w.tau[0][:, 0, :][w.carrier[:, 0, :]] == dtype(-nu * gamma)).all()
    # the x and z lines of this block are open runs (no closing cell): they expose nothing
    assert not w.carrier[~(plate | (ty != NODE_IN))].any()
    for a in w.tau + [w.mag, w.q, w.area]:
        assert a.dtype == np.dtype(dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_linear_temperature_gives_the_heat_flux(dtype):
    dims = (6, 4, 4)
    ty, bv, bt = fluid_block(dims)
    ty[0], ty[5] = NODE_BOUND, NODE_BOUND
    G, kappa = 4.0, 0.125
    T = np.broadcast_to((G * np.arange(6) * POW2[0])[:, None, None], dims).astype(dtype)
    zero = np.zeros(dims, dtype)
    w = LO.wall_loads((ty, bv, bt), [zero, zero, zero, T], POW2, 1.0, kappa)
    assert w.carrier[0].all() and w.carrier[5].all() and w.carrier.sum() == 2 * 16
    assert (w.q[0] == dtype(kappa * G)).all(), "the fluid is warmer than the wall: heat flows into it"
    assert (w.q[5] == dtype(-kappa * G)).all()
    assert not w.mag.any()
    bt[0] = BC_FREE                                            # a FREE temperature face: its area counts, its flux does not
    w = LO.wall_loads((ty, bv, bt), [zero, zero, zero, T], POW2, 1.0, kappa)
    assert w.carrier[0].all() and not w.q[0].any() and (w.area[0] == dtype(POW2[1] * POW2[2])).all()


@pytest.mark.parametrize("dtype", DTYPES)
def test_single_wall_cell_takes_the_area_weighted_mean(dtype):
    dims = (7, 7, 7)
    ty, bv, bt = fluid_block(dims)
    for a in range(3):                                         # the shell closes every line
        sl = [slice(None)] * 3
        for e in (0, 6):
            sl[a] = e
            ty[tuple(sl)] = NODE_BOUND
    ty[3, 3, 3] = NODE_BOUND
    rng = np.random.default_rng(3)
    F = [rng.integers(-8, 9, dims).astype(dtype) for _ in range(4)]
    nu, kappa = 0.5, 2.0
    w = LO.wall_loads((ty, bv, bt), F, POW2, nu, kappa)
    faces = LO.exposed_faces(ty)
    assert all(f[3, 3, 3] for f in faces), "six exposed faces"
    h = POW2
    A = [h[1] * h[2], h[0] * h[2], h[0] * h[1]]
    B_ = (3, 3, 3)
    want = np.zeros(4)
    for d in range(3):
        for s in (-1, 1):
            P = tuple(B_[a] + (s if a == d else 0) for a in range(3))
            for c in range(4):
                if c != d:
                    want[c] += A[d] * (kappa if c == 3 else nu) * (float(F[c][P]) - float(F[c][B_])) / h[d]
    area = 2 * sum(A)
    assert w.area[B_] == dtype(area)
    for c in range(3):
        assert w.tau[c][B_] == dtype(want[c] / area)           # (small integers and powers of two: every operation is exact)
    assert w.q[B_] == dtype(want[3] / area)


def test_free_outflow_face_is_a_carrier_with_zero_loads():
    n = grids.box(8, 6, 7)
    rng = np.random.default_rng(4)
    F = [rng.uniform(1, 2, n.shape).astype(np.float32) for _ in range(4)]
    w = LO.wall_loads(n, F, (n.dx, n.dy, n.dz), 0.3, 0.2)
    out = np.zeros(n.shape, bool)
    out[-1, 1:-1, 1:-1] = True
    assert w.carrier[out].all() and (w.area[out] > 0).all()
    assert not any(w.tau[c][out].any() for c in range(3)) and not w.q[out].any() and not w.mag[out].any()
    # the shell is NOSLIP for the velocity and FREE for the temperature: shear and no flux; the inflow valve has both
    shell = w.carrier & (np.asarray(n.type) == NODE_BOUND)
    assert w.mag[shell].any() and not w.q[shell].any() and w.q[0, 1:-1, 1:-1].all()
    # the records: 99999 on NODE_OUT, 0 on the cells that are no carriers, the loads on the carriers
    n.type[2:4, 2:4, 2:4] = NODE_OUT
    V, T = LO.layer_output(n, F, vector=LO.WALL_SCALARS, spacing=(n.dx, n.dy, n.dz), nu=0.3, kappa=0.2)
    w = LO.wall_loads(n, F, (n.dx, n.dy, n.dz), 0.3, 0.2)
    assert (V[2:4, 2:4, 2:4] == np.float32(99999.0)).all() and (T[2:4, 2:4, 2:4] == 99999.0).all()
    assert not w.carrier[2:4, 2:4, 2:4].any(), "NODE_OUT next to NODE_IN is no carrier"
    quiet = ~w.carrier & (np.asarray(n.type) != NODE_OUT)
    assert not V[quiet].any() and np.array_equal(V[w.carrier, 0], w.mag[w.carrier]) and np.array_equal(V[w.carrier, 2], w.area[w.carrier])
    Vv, _ = LO.layer_output(n, F, vector=LO.WALL_VECTOR, spacing=(n.dx, n.dy, n.dz), nu=0.3, kappa=0.2)
    assert all(np.array_equal(Vv[w.carrier, c], w.tau[c][w.carrier]) for c in range(3))
    assert np.array_equal(T[quiet | w.carrier], F[3][quiet | w.carrier].astype(np.float64)), "the fourth quantity stays the temperature"


@pytest.mark.parametrize("dtype", DTYPES)
def test_steady_and_alternating_windows(dtype):
    n = grids.box_with_obstacle(9, 8, 7)
    spacing = POW2
    rng = np.random.default_rng(6)
    F = [rng.integers(-8, 9, n.shape).astype(dtype) for _ in range(4)]
    w = LO.wall_loads(n, F, spacing, 0.5, 0.25)
    steady = TS.TimeStats(n.shape, 1, wall=True, spacing=spacing, nu=0.5, kappa=0.25)
    for _ in range(4):
        steady.add(F, n)
    assert np.array_equal(steady.nw, np.where(w.carrier, 4, 0))
    Q3, Q4 = steady.wall_layer(F, 3), steady.wall_layer(F, 4)
    on = w.carrier
    assert all(np.array_equal(Q3[c][on], w.tau[c][on]) for c in range(3))
    assert np.array_equal(Q4[0][on], w.mag[on]), "tawss of a steady window is mag"
    assert np.array_equal(Q4[1][on], w.q[on])
    # OSI 0: to the rounding of |mean tau| against mean |tau| (mag is rounded in R, the mean's magnitude in double)
    assert (Q4[2][on] <= 4 * np.finfo(dtype).eps).all() and (Q4[2] >= 0).all()
    assert not any(q[~on].any() for q in Q3[:3] + Q4[:3])
    assert np.array_equal(Q3[3], steady.layer(TS.MEAN, F)[3]) and np.array_equal(Q4[3], Q3[3])
    # a flow whose sign alternates every step: the mean traction vanishes, the mean magnitude does not
    alt = TS.TimeStats(n.shape, 1, wall=True, spacing=spacing, nu=0.5, kappa=0.25)
    for k in range(4):
        alt.add([f if k % 2 == 0 else -f for f in F], n)
    Q4 = alt.wall_layer(F, 4)
    sheared = on & (w.mag > 0)
    assert sheared.any() and (Q4[2][sheared] == dtype(0.5)).all() and np.array_equal(Q4[0][on], w.mag[on])
    assert not Q4[2][on & (w.mag == 0)].any(), "tawss = 0: OSI 0"
    assert not any(q[on].any() for q in alt.wall_layer(F, 3)[:3])


# ---- the exposed-face rule against the line walk ----

def random_types(dims, seed):
    rng = np.random.default_rng(seed)
    ty = rng.choice(np.array([NODE_IN, NODE_OUT, NODE_BOUND, NODE_VALVE], np.uint8), size=dims, p=[0.55, 0.12, 0.23, 0.10])
    ty[1, 1, :4] = [NODE_IN, NODE_BOUND, NODE_IN, NODE_BOUND]   # an IN-typed first cell of a z line, then a wall
    ty[2, 2, -4:] = [NODE_BOUND, NODE_IN, NODE_IN, NODE_IN]     # an open fluid run that reaches the grid edge
    ty[3, 1, 1:6] = [NODE_VALVE, NODE_IN, NODE_BOUND, NODE_IN, NODE_VALVE]       # a one-cell wall between two fluid runs
    ty[0, 3, 1:5] = [NODE_BOUND, NODE_IN, NODE_OUT, NODE_IN]    # NODE_OUT next to NODE_IN
    return ty


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_exposed_faces_against_the_line_walk(seed):
    dims = (6, 5, 9)
    ty = random_types(dims, seed)
    faces, kinds = walked_faces(ty)
    got = LO.exposed_faces(ty)
    for n in range(6):
        assert np.array_equal(got[n], faces[n]), n
    assert sum(int(f.sum()) for f in faces) > 50
    # the cases the rule is about
    assert not got[4][1, 1, 1] and got[5][1, 1, 1] and ty[1, 1, 0] == NODE_IN, "an IN-typed first cell of a line: no face towards it"
    assert not got[5][2, 2, dims[2] - 4], "an open run to the grid edge: no face"
    assert got[4][3, 1, 3] and got[5][3, 1, 3] and kinds[2][3, 1, 3] == START, "the shared START/END cell: both faces count"
    assert got[5][0, 3, 1], "a run closed by a NODE_OUT cell"
    carrier = np.logical_or.reduce(got)
    assert not carrier[ty == NODE_OUT].any() and not carrier[ty == NODE_IN].any()
    assert carrier[ty == NODE_VALVE].any() and carrier[ty == NODE_BOUND].any()
    # what the kernel tests instead: s = -1 -- the cell below is NODE_IN and not the first of its line; s = +1 -- the wall cell's
    # row kind is START; and then its kind is START or END, so its nibble carries the FREE bits
    wall = (ty == NODE_BOUND) | (ty == NODE_VALVE)
    for d in range(3):
        t = np.moveaxis(ty, d, 0)
        below_in = np.zeros(t.shape, bool)
        below_in[2:] = t[1:-1] == NODE_IN
        assert np.array_equal(np.moveaxis(below_in, 0, d) & wall, got[2 * d])
        assert np.array_equal((kinds[d] == START) & wall, got[2 * d + 1])
        ends = (kinds[d] == START) | (kinds[d] == END)
        assert ends[got[2 * d] | got[2 * d + 1]].all()


@pytest.mark.parametrize("dtype", DTYPES)
def test_loads_against_the_cell_loop(dtype):
    dims = (6, 5, 9)
    ty = random_types(dims, 7)
    rng = np.random.default_rng(8)
    bv, bt = (rng.random(dims) < 0.3).astype(np.uint8), (rng.random(dims) < 0.3).astype(np.uint8)
    F = [rng.uniform(-3, 3, dims).astype(dtype) for _ in range(4)]
    spacing, nu, kappa = (0.3, 0.07, 0.11), 0.013, 0.021
    carrier, want = loop_loads((ty, bv, bt), F, spacing, nu, kappa)
    w = LO.wall_loads((ty, bv, bt), F, spacing, nu, kappa)
    assert np.array_equal(w.carrier, carrier) and carrier.sum() > 30
    for got, ref in zip(w.tau + [w.mag, w.q, w.area], want):
        assert got.dtype == np.dtype(dtype) and np.array_equal(got, ref)
    # filter 1 averages over the carriers of a box; an empty box gives the point sample
    V, T = LO.layer_output((ty, bv, bt), F, (3, 2, 4), LO.BOX, LO.WALL_VECTOR, spacing, nu=nu, kappa=kappa, exact_sum=True)
    q = LO.cell_quantities((ty, bv, bt), F, LO.WALL_VECTOR, spacing, nu, kappa)
    ax = [LO.boxes(g, o) for g, o in zip(dims, (3, 2, 4))]
    for i in range(3):
        for j in range(2):
            for k in range(4):
                box = tuple(slice(int(a[0][m]), int(a[1][m])) for a, m in zip(ax, (i, j, k)))
                m = carrier[box]
                for c in range(3):
                    if m.any():
                        vals = q[c][box][m].astype(np.float64)
                        assert V[i, j, k, c] == dtype(math.fsum(vals) / float(m.sum()))
                    else:
                        assert V[i, j, k, c] == q[c][box][0, 0, 0]


def test_time_sums_follow_a_moving_geometry_and_the_stride():
    dims = (13, 11, 10)
    spacing = (0.3, 0.07, 0.11)
    A, Bn = grids.box_with_obstacle(*dims, lo=0.25, hi=0.6), grids.box_with_obstacle(*dims, lo=0.4, hi=0.75)
    rng = np.random.default_rng(5)
    steps = [([rng.uniform(-2, 2, dims).astype(np.float32) for _ in range(4)], Bn if k in (2, 3) else A) for k in range(5)]
    for every in (1, 2):
        ts = TS.TimeStats(dims, 1, every=every, wall=True, spacing=spacing, nu=0.01, kappa=0.02)
        nw = np.zeros(dims, np.uint32)
        W = [np.zeros(dims, np.float64) for _ in range(5)]
        for k, (fields, nodes) in enumerate(steps):
            assert ts.add(fields, nodes) == (k % every == 0)
            if k % every:
                continue
            w = LO.wall_loads(nodes, fields, spacing, 0.01, 0.02)
            nw += w.carrier.astype(np.uint32)
            for v, a in enumerate(w.tau + [w.mag, w.q]):
                W[v] = np.where(w.carrier, W[v] + a.astype(np.float64), W[v])
        assert np.array_equal(ts.nw, nw) and all(np.array_equal(a, b) for a, b in zip(ts.W, W))
        assert 0 < nw.max() == ts.N and nw[nw > 0].min() < ts.N, "carriers that come and go"
    ts.reset()
    assert ts.N == 0 and not ts.nw.any() and not any(w.any() for w in ts.W)


def test_refusals_of_the_twin():
    dims = (5, 5, 5)
    n = grids.box(*dims)
    fields = [np.ones(dims, np.float32)] * 4
    with pytest.raises(ValueError):
        TS.TimeStats(dims, 1, wall=True, spacing=POW2)             # no nu, kappa
    plain = TS.TimeStats(dims, 1)
    assert plain.nw is None and plain.W is None
    plain.add(fields, np.asarray(n.type))
    with pytest.raises(ValueError):
        plain.wall_layer(fields, 3)                                # the window holds no wall sums
    ts = TS.TimeStats(dims, 1, wall=True, spacing=POW2, nu=1.0, kappa=1.0)
    with pytest.raises(ValueError):
        ts.wall_layer(fields, 4)                                   # no step yet
    ts.add(fields, n)
    with pytest.raises(ValueError):
        ts.wall_layer(fields, 2)
    with pytest.raises(ValueError):
        LO.layer_output(n, fields, vector=LO.WALL_VECTOR, spacing=POW2)            # no nu, kappa
    with pytest.raises(ValueError):
        LO.layer_output(np.asarray(n.type), fields, vector=LO.WALL_VECTOR, spacing=POW2, nu=1.0, kappa=1.0)      # no boundary conditions


def test_driver_refuses_time_wall_when_it_reads_the_arguments(built, tmp_path):
    driver = B.build_driver()
    data, cfgf = (os.path.join(INPUTS, f) for f in ("box_pipe_2D_data.txt", "box_pipe_2D_config.txt"))
    prefix = str(tmp_path / "o")
    for words, text in ((["GPU", "--time-wall"], "--time-wall: needs --time-stats"),
                        (["GPU", "--time-wall", "--output-filter", "box"], "--time-wall: needs --time-stats"),
                        (["GPU", "2", "--time-stats", "mean", "--time-wall"], "--time-wall: single GPU only"),
                        (["--time-stats", "variance", "--time-gradients", "--time-wall", "GPU", "2"], "single GPU only")):
        r = subprocess.run([driver, data, prefix, cfgf, "align"] + words, capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and text in r.stderr, words
        assert "Grid =" not in r.stdout, "refused before the geometry is loaded"
        assert not os.path.exists(prefix + "_res.nc") and not os.path.exists(prefix + "_stats.nc")
    usage = subprocess.run([driver], capture_output=True, text=True, timeout=60).stdout
    assert "[--time-wall]" in usage
