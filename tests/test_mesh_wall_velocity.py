"""Walls of a Shape3D mesh that carry the mesh's velocity (conservative voxelisation): the twin's owner against an independent
painting, its weights against a least-squares projection, the two velocity sources of the loaders, the C++ loader against the twin
byte for byte (fs3d_run --grid-only) and the physics of a translating sphere on the CPU oracle alone."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import abi_decls  # noqa: E402
import mesh_cases as MC  # noqa: E402
import wall_velocity_cases as WV  # noqa: E402
import watertight_cases as W  # noqa: E402
from test_gpu_moving import INPUTS, PARAMS, clear_oracle  # noqa: E402
from test_shape3d import _grid_dump, icosphere  # noqa: E402
from cmc_fluid_solver_amd import build as B  # noqa: E402
from cmc_fluid_solver_amd import capi, grids, shape2d, shape3d  # noqa: E402

ROUNDING = 2.0 ** -48          # under ten float64 roundings of 2^-53, with a margin of three


# ---- 1. the owner ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", WV.CPU_OWNER_CASES)
def test_owner_is_the_smallest_index_and_follows_a_reversed_list(case):
    sh, g, idx = WV.mesh(case)
    changed = []
    for tri in (idx, idx[::-1].copy()):
        tw = WV.built(sh, g, tri, None)
        own = WV.painted_owner(sh, g, tri)
        assert np.array_equal(tw.owner, own), "%d cells" % int((tw.owner != own).sum())
        assert np.array_equal(tw.owner != shape3d.NO_OWNER, tw.type == grids.NODE_BOUND)
        changed.append(np.where(own >= 0, len(tri) - 1 - own, -1) if tri is not idx else own)
    # the same triangles under other indices: some cell is overlapped by several, and its owner is another triangle now
    assert (changed[0] != changed[1]).any()


# ---- 2. the interpolation ----------------------------------------------------------------------------------------------------------

def wall_cells(tw):
    return np.nonzero(tw.type == grids.NODE_BOUND)


@pytest.mark.parametrize("case", ["sphere-20", "tetra", "ragged", "outside", "degenerate"])
def test_wall_values_lie_within_the_owner_s_vertex_values(case):
    sh, g, idx = WV.mesh(case)
    vel = WV.velocities(g)
    tw = WV.built(sh, g, idx, vel)
    ci, cj, ck = wall_cells(tw)
    assert len(ci) > 0
    W3 = vel[idx[tw.owner[ci, cj, ck]]].astype(np.float64)          # [cells, vertex, component]
    tol = ROUNDING * float(np.abs(vel).max())
    for c in range(3):
        u = tw.wall_v[c][ci, cj, ck]
        assert (u >= W3[:, :, c].min(1) - tol).all() and (u <= W3[:, :, c].max(1) + tol).all()
        assert not tw.wall_v[c][tw.type != grids.NODE_BOUND].any()
    assert len(np.unique(tw.wall_v[0][ci, cj, ck])) > len(ci) // 4      # (the field is not uniform)


@pytest.mark.parametrize("case", ["sphere-20", "tetra", "degenerate"])
def test_a_uniform_velocity_comes_back(case):
    sh, g, idx = WV.mesh(case)
    U = np.array([0.3, -1.7, 0.011], np.float32)
    tw = WV.built(sh, g, idx, np.tile(U, (len(g), 1)))
    ci, cj, ck = wall_cells(tw)
    for c in range(3):
        assert np.abs(tw.wall_v[c][ci, cj, ck] - float(U[c])).max() <= ROUNDING * float(np.abs(U).max())


@pytest.mark.parametrize("case", ["sphere-20", "tetra", "box_pipe_3D"])
def test_an_affine_field_is_reproduced_at_the_centre_s_projection(case):
    """Where the projection of the cell's centre falls inside the owner (all three unclamped weights positive) the rule gives the
    affine field at that point: to 1e-9 (|A| extent + |b|) with the field's exact float64 vertex values through wall_weights /
    wall_velocity, and -- the arrays build() keeps come from the fp32 vertex velocities, each within 2^-24 of its value, and the
    weights are convex -- to that plus 2^-24 max |W| there."""
    sh, g, idx = WV.mesh(case)
    A, b = WV.affine()
    vel = WV.velocities(g)
    tw = WV.built(sh, g, idx, vel)
    ci, cj, ck = wall_cells(tw)
    step = max(1, len(ci) // 400)                                     # a few hundred cells spread over the surface
    extent = float(max(tw.type.shape))
    tol = 1e-9 * (np.abs(A).sum(1).max() * extent + np.abs(b).max())
    checked = 0
    for i, j, k in zip(ci[::step], cj[::step], ck[::step]):
        t = tw.owner[i, j, k]
        p = g[idx[t]].astype(np.float64)
        point, bary = WV.projection(p, np.array([i, j, k], np.float64) + 0.5)
        if not (bary > 1e-6).all():
            continue
        want = A @ point + b
        w = shape3d.wall_weights([[np.float32(x) for x in v] for v in g[idx[t]]], (i, j, k))
        assert np.abs(np.array(w) - bary).max() <= 1e-9
        exact = shape3d.wall_velocity(w, p @ A.T + b)
        assert np.abs(np.array(exact) - want).max() <= tol
        got = np.array([tw.wall_v[c][i, j, k] for c in range(3)])
        assert np.abs(got - want).max() <= tol + 2.0 ** -24 * float(np.abs(vel).max())
        checked += 1
    assert checked >= 20, checked


@pytest.mark.parametrize("name", list(W.DEGENERATE))
def test_a_degenerate_owner_gives_the_clamped_edge_parameter(name):
    tri, (a, e) = W.DEGENERATE[name]
    sh = W.blank(W.DEGENERATE_DIMS)
    g = np.array(tri, np.float32)
    vel = np.array([[1.0, 10.0, 100.0], [2.0, 20.0, 200.0], [4.0, 40.0, 400.0]], np.float32)
    tw = WV.built(sh, g, np.array([[0, 1, 2]]), vel)
    ci, cj, ck = wall_cells(tw)
    assert len(ci) > 0
    a, e = np.array(a, np.float64), np.array(e, np.float64)
    # the two ends of the longest edge among the triangle's vertices (the first edge of equal ones: (0,1), (1,2), (2,0))
    d2 = [float(((g[j].astype(np.float64) - g[i]) ** 2).sum()) for i, j in ((0, 1), (1, 2), (2, 0))]
    first = int(np.argmax(d2))                                       # (argmax returns the first of equals)
    v0, v1 = first, (first + 1) % 3
    assert {tuple(g[v0]), tuple(g[v1])} == {tuple(a.astype(np.float32)), tuple(e.astype(np.float32))}
    p0, p1 = g[v0].astype(np.float64), g[v1].astype(np.float64)
    ll = float(((p1 - p0) ** 2).sum())
    for i, j, k in zip(ci, cj, ck):
        c = np.array([i, j, k], np.float64) + 0.5
        t = min(max(float((c - p0) @ (p1 - p0)) / ll, 0.0), 1.0) if ll > 0 else 0.0
        want = (1 - t) * vel[v0].astype(np.float64) + t * vel[v1].astype(np.float64)
        got = np.array([tw.wall_v[q][i, j, k] for q in range(3)])
        assert np.abs(got - want).max() <= 2 * ROUNDING * float(np.abs(vel).max()), (i, j, k, t, got, want)


# ---- 3. where the loaders take vertex velocities from ---------------------------------------------------------------------------

def two_frame_text(columns):
    v, f = icosphere(6.0, (20.0, 21.0, 22.0), subdiv=0)
    v2 = v + np.array([1.0, -0.25, 0.5])
    rng = np.random.default_rng(11)
    txt = "2\n"
    for fr in (v, v2):
        w = rng.uniform(-2, 2, fr.shape) if columns else np.zeros(fr.shape)
        txt += "%d\n" % len(fr) + "".join("%.6g %.6g %.6g %.6g %.6g %.6g\n" % (tuple(p) + tuple(q)) for p, q in zip(fr, w))
        txt += "%d\n" % len(f) + "".join("%d %d %d\n" % tuple(t) for t in f)
    return txt


def test_motion_velocities_are_the_displacement_rate_and_wrap():
    F = np.float32
    sh = shape3d.Shape3D(shape3d.parse_shape3d(two_frame_text(False)), 0.001, 0.001, 0.001, False, voxels="conservative")
    f0, f1 = sh.frames
    dur = 1.0 / 75
    for t, (a, b) in ((0.004, (f0, f1)), (dur + 0.004, (f1, f0))):          # the last frame's successor is frame 0
        w = sh.subframe_velocity(t, "motion")
        assert w.dtype == np.float32
        want = ((b["v"] - a["v"]).astype(F) * F(1.0 / dur)).astype(F)
        assert np.array_equal(w, want) and np.abs(w).max() > 0
        # velocity x duration is the displacement, to the two fp32 roundings of the expression
        disp = (b["v"].astype(np.float64) - a["v"])
        assert np.abs(w.astype(np.float64) * dur - disp).max() <= 2.0 ** -22 * np.abs(disp).max()
    assert np.abs(sh.subframe_velocity(0.004, "motion")[:, 0] - 0.075).max() < 1e-6      # 1 mm in 1/75 s
    one = shape3d.Shape3D(shape3d.parse_shape3d(W.sphere_text(20, (15, 19, 15))[0]), 0.001, 0.001, 0.001, False, voxels="conservative")
    assert not one.subframe_velocity(0.004, "motion").any()


def test_file_velocities_are_the_reference_s_interpolation():
    F = np.float32
    sh = shape3d.Shape3D(shape3d.parse_shape3d(two_frame_text(True)), 0.001, 0.001, 0.001, False, voxels="conservative")
    f0, f1 = sh.frames
    dur = 1.0 / 75
    for t, (a, b) in ((0.004, (f0, f1)), (dur + 0.009, (f1, f0))):
        s = F((t - (0.0 if a is f0 else dur)) / dur)
        want = ((a["vel"] * F(F(1) - s)).astype(F) + (b["vel"] * s).astype(F)).astype(F)
        got = sh.subframe_velocity(t, "file")
        assert np.array_equal(got, want) and np.abs(got).max() > 0.5
    with pytest.raises(ValueError):
        sh.subframe_velocity(0.0, "rest")
    with pytest.raises(ValueError):
        shape3d.Shape3D(shape3d.parse_shape3d(two_frame_text(True)), 0.001, 0.001, 0.001, False, wall_velocity="motion")      # needs conservative


# ---- 4. the C++ loader against the twin --------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def driver(built):
    return B.build_driver()


@pytest.fixture(scope="module")
def sphere_with_columns(tmp_path_factory):
    """sphere_3D with non-zero velocity columns (the shipped file's are zero), for the `file` source"""
    src = open(os.path.join(INPUTS, "sphere_3D_data.txt")).read().split()
    rng = np.random.default_rng(5)
    it = iter(src)
    out = [next(it)]
    for _ in range(int(out[0])):
        nv = next(it); out.append(nv)
        for _ in range(int(nv)):
            out += [next(it), next(it), next(it)] + ["%.5f" % x for x in rng.uniform(-0.2, 0.2, 3)]
            next(it); next(it); next(it)
        nt = next(it); out.append(nt)
        out += [next(it) for _ in range(3 * int(nt))]
    path = str(tmp_path_factory.mktemp("wallvel") / "sphere_cols_3D_data.txt")
    open(path, "w").write("\n".join(out) + "\n")
    return path


GRID_TIMES = (0.004, 0.0131, 0.0187)          # frames of 1/75 s: two times in frame 0, one in frame 1 (whose successor is frame 0)


@pytest.mark.parametrize("prec", ["float", "double"])
@pytest.mark.parametrize("source", ["motion", "file", "file-columns"])
def test_cpp_loader_equals_the_twin_with_moving_walls(driver, sphere_with_columns, tmp_path, source, prec):
    cfgf = os.path.join(INPUTS, "sphere_3D_config.txt")
    data = sphere_with_columns if source == "file-columns" else os.path.join(INPUTS, "sphere_3D_data.txt")
    word = source.split("-")[0]
    cfg = shape2d.Config(cfgf)
    dtype = np.float32 if prec == "float" else np.float64
    moving_cells = 0
    for t in GRID_TIMES:
        dump = str(tmp_path / ("grid_%g.bin" % t))
        args = [driver, data, str(tmp_path / "out"), cfgf, "align", "--watertight", "--wall-velocity", word, "--wall-temperature", "1",
                "--grid-only", dump, "--grid-time", repr(t)] + (["double"] if prec == "double" else [])
        subprocess.run(args, check=True, capture_output=True, text=True)
        nodes, sh = shape3d.load_shape3d(data, cfg.dx, cfg.dy, cfg.dz, cfg.baseT, True, voxels="conservative", wall_velocity=word, wall_T=1.0, time=t)
        got = _grid_dump(dump)
        for name in MC.NODE_ARRAYS:
            want = np.ascontiguousarray(getattr(nodes, name), got[name].dtype)
            assert got[name].shape == want.shape
            assert np.array_equal(got[name].view(np.uint8), want.view(np.uint8)), (name, t, int((got[name] != want).sum()))
        assert got["vx"].dtype == dtype and (got["T"][got["type"] == grids.NODE_BOUND] == 1).all()
        moving_cells += int((got["vx"] != 0).sum())
    assert (moving_cells > 0) == (source != "file")          # (the shipped sphere's velocity columns are zero)


def test_driver_refuses_wall_velocity_without_watertight(driver, tmp_path):
    data, cfgf = (os.path.join(INPUTS, f) for f in ("sphere_3D_data.txt", "sphere_3D_config.txt"))
    r = subprocess.run([driver, data, str(tmp_path / "o"), cfgf, "align", "--wall-velocity", "motion", "--grid-only", str(tmp_path / "g.bin")],
                       capture_output=True, text=True)
    assert r.returncode != 0 and "--watertight" in r.stderr
    r = subprocess.run([driver, data, str(tmp_path / "o"), cfgf, "align", "--watertight", "--wall-velocity", "fast", "--grid-only", str(tmp_path / "g.bin")],
                       capture_output=True, text=True)
    assert r.returncode != 0 and "motion or file" in r.stderr


def test_zero_velocities_and_wall_temperature_zero_are_today_s_nodes():
    sh, g, idx = WV.mesh("sphere-20")
    a = WV.nodes_of(WV.built(sh, g, idx, np.zeros(g.shape, np.float32)), 0.0)
    b = MC.nodes_of(W.conservative(sh, g, idx))
    for name in MC.NODE_ARRAYS:
        assert np.array_equal(np.asarray(getattr(a, name)).view(np.uint8), np.asarray(getattr(b, name)).view(np.uint8)), name


# ---- 5. the physics, on the CPU oracle alone -----------------------------------------------------------------------------------------

def oracle_run(speed):
    from oracle import oracle as O
    dtype = np.float32
    steps = WV.translating_grids(speed)
    params = capi.fluid_params(dtype, *PARAMS)
    o = O.Oracle(steps[0][0], params, dtype)
    errs = []
    for nodes, _, _, _ in steps:
        rc, err = WV.oracle_step(O, o, nodes, dtype, clear_oracle)
        assert rc == 0
        errs.append(err)
    u = np.asarray(o.get_layer_fields(O.L_CUR)[0], np.float64)
    inside = steps[-1][0].type == grids.NODE_IN
    assert inside.sum() > 100
    o.close()
    return errs, u, inside


def test_a_translating_sphere_carries_its_fluid_along(built):
    errs, u, inside = oracle_run(WV.WALL_SPEED)
    mean_u = float(u[inside].mean())
    print("reported errors", errs, "mean u over NODE_IN", mean_u, "wall speed", WV.WALL_SPEED)
    assert max(errs) < 0.01
    assert mean_u >= 0.9 * WV.WALL_SPEED


def test_the_same_sphere_with_walls_at_rest_leaves_the_fluid_alone(built):
    errs, u, inside = oracle_run(0.0)
    print("reported errors", errs, "largest |u|", float(np.abs(u).max()))
    assert max(errs) < 0.01
    assert float(np.abs(u).max()) <= 1e-6


def test_sphere_3D_with_moving_walls_stays_below_the_error_threshold(built):
    """The driver's moving-mesh run of tests/test_gpu_mesh_wall_velocity.py on the CPU oracle, through the twin's grids: sphere_3D
    moves 1 mm in x and 0.5 mm in z per frame, 0.075 m/s and half of it; with `--wall-velocity motion --wall-temperature 1` the
    reported error of every step stays below the solver's 0.01 threshold."""
    from oracle import oracle as O
    dtype = np.float32
    data, cfgf = (os.path.join(INPUTS, f) for f in ("sphere_3D_data.txt", "sphere_3D_config.txt"))
    cfg = shape2d.Config(cfgf)
    nodes, sh = shape3d.load_shape3d(data, cfg.dx, cfg.dy, cfg.dz, cfg.baseT, True, voxels="conservative", wall_velocity="motion", wall_T=1.0)
    w = sh.subframe_velocity(0.0, "motion")
    assert abs(float(w[0, 0]) - 0.075) < 1e-5 and abs(float(w[0, 2]) - 0.0375) < 1e-5 and not w[:, 1].any()
    dt = cfg.frame_time / (len(sh.frames) * cfg.time_steps)
    final = cfg.frame_time * cfg.cycles
    o = O.Oracle(nodes, capi.fluid_params(dtype, cfg.Re, cfg.Pr, cfg.lam), dtype)
    t, errs = dt, []
    while t < final:
        sh.prepare(t)
        now = shape3d.nodes_of(sh, cfg.dx, cfg.dy, cfg.dz, cfg.baseT, sh.wall_v, 1.0)
        o._f("fs3d_oracle_set_nodes")(o.h, *[O._ptr(x) for x in WV.oracle_arrays(now, dtype)])
        o._f("fs3d_oracle_create_segments")(o.h)
        o.update_boundaries()
        rc, err = o.time_step(float(dtype(dt)), cfg.num_global, cfg.num_local, True)
        assert rc == 0
        errs.append(err)
        clear_oracle(o, now.type == grids.NODE_OUT, cfg.baseT)
        t += dt
    print("reported errors", errs)
    assert len(errs) in (7, 8) and max(errs) < 0.01
    o.close()


# ---- the declarations --------------------------------------------------------------------------------------------------------------

def test_the_header_the_binding_and_the_library_agree(built):
    """include/fs3d.h declares the two entries, capi.SYMBOLS binds them, the library exports them."""
    lib = ctypes.CDLL(capi.LIB_PATH)
    for name in ("fs3d_update_nodes_shape3d_vel", "fs3d_voxelize_shape3d_vel_dev"):
        assert abi_decls.declares_status(name), name
        assert hasattr(lib, name), "libfs3d_hip.so does not export %s" % name
        assert getattr(capi.load(), name).argtypes == capi.SYMBOLS[name][1]
        assert callable(getattr(capi.Solver, name[len("fs3d_"):]))
