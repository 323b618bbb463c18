"""Meshes and grids of the Shape3D voxeliser tests (tests/test_mesh_api.py, tests/test_gpu_mesh.py): every case is
(Shape3D twin holding the expected grid, vertices in grid coordinates, triangles, the reference's own type array or None).
The expected grids come from cmc_fluid_solver_amd/shape3d.py alone, which tests/test_ref_golden.py pins to the reference."""
import functools
import os

import numpy as np
from scipy import ndimage

import refgolden as RG
from cmc_fluid_solver_amd import grids, shape3d

BASE_T = 1.0
NODE_ARRAYS = ("type", "bc_vel", "bc_temp", "vx", "vy", "vz", "T")
CASE_IDS = ["sphere-t0", "sphere-t1", "sphere-t2", "sphere-t3", "sphere-t4", "box_pipe_3D", "tetra", "sphere-ragged", "sphere-outside",
            "sphere-degenerate"]


def twin(name, align=True, time=0.0):
    fx = RG.Fixture(name, "f32")
    cfg = fx.cfg()
    return shape3d.Shape3D(shape3d.parse_shape3d(open(fx.data_path).read()), cfg.dx, cfg.dy, cfg.dz, align, time), fx


@functools.lru_cache(maxsize=None)
def load_case(case):
    if case.startswith("sphere-t"):
        k = int(case[-1])
        sh, fx = twin("sphere_3D", time=fx_times()[k])
        g, idx = sh.subframe(fx_times()[k])
        return sh, g, idx, fx.z["grid%d_type" % k]
    if case in ("box_pipe_3D", "tetra"):
        sh, fx = twin(case)
        g, idx = sh.subframe(0.0)
        return sh, g, idx, fx.z["node_type"]
    if case == "sphere-ragged":                 # no `align`: ragged dims, dimz % 4 != 0 -- one cell per thread in the node kernel
        sh, fx = twin("sphere_3D", align=False)
        assert sh.dimz % 4 != 0, sh.type.shape
        g, idx = sh.subframe(0.0)
        return sh, g, idx, None
    sh, fx = twin("sphere_3D")
    g, idx = sh.subframe(0.0)
    if case == "sphere-outside":                # partly outside the grid, on the negative side of x and past the end of z
        g = (g + np.array([-9.3, 4.7, 20.2], np.float32)).astype(np.float32)
        assert g[:, 0].min() < -1 and g[:, 2].max() > sh.dimz + 1
    else:                                       # three equal vertices, and three collinear ones (a zero normal): edge lines only
        g = np.concatenate([g, np.array([[1, 1, 1], [3, 3, 3], [5, 5, 5]], np.float32)])
        n = len(g)
        idx = np.concatenate([idx, [[0, 0, 0], [n - 3, n - 2, n - 1]]])
    sh.build(g, idx)
    return sh, g, idx, None


def fx_times():
    return RG.Fixture("sphere_3D", "f32").meta["grid_times"]


def nodes_of(sh):
    return shape3d.nodes_of(sh, sh.dx, sh.dy, sh.dz, BASE_T)


def long_scan_line_mesh():
    """One triangle in the plane z = 3 whose scan lines along x are 120 000 cells long: finite, inside the coordinate bound, and
    far past 4 (dimx + dimy + dimz) + 16 cells of a 32^3 grid."""
    return np.array([[-60000.0, -5.0, 3.0], [60000.0, -5.5, 3.0], [0.0, 50.0, 3.0]], np.float32), np.array([[0, 1, 2]])


# ---- flood fill ---------------------------------------------------------------------------------------------------------------

def label_fill(ty):
    """FloodFill (Grid3D.cpp:813-857) as a connected component: what every implementation must give."""
    free = ty == grids.NODE_IN
    free[0, 0, 0] = True
    lab, _ = ndimage.label(free)
    out = ty.copy()
    out[lab == lab[0, 0, 0]] = grids.NODE_OUT
    return out


def serpentine(dims=(24, 20, 70)):
    """Walls across x at every second plane, each with one hole in alternating corners (the far z corner lies in the second 64-cell
    chunk of a Z line): NODE_OUT has to snake through every slab.  Slabs carry a baffle along y with a hole of its own, two hold
    a closed box whose inside must stay NODE_IN, and the last slab is sealed."""
    nx, ny, nz = dims
    ty = np.full(dims, grids.NODE_IN, np.uint8)
    for n, x in enumerate(range(2, nx - 3, 2)):
        ty[x] = grids.NODE_BOUND
        ty[x, 0 if n % 2 else ny - 1, nz - 1 if n % 3 else 0] = grids.NODE_IN
        ty[x + 1, ny // 2, :] = grids.NODE_BOUND
        ty[x + 1, ny // 2, (7 * n) % nz] = grids.NODE_IN
    ty[nx - 3] = grids.NODE_BOUND
    for x in (1, 5):
        ty[x, 2:7, 60:68] = grids.NODE_BOUND
        ty[x, 3:6, 61:67] = grids.NODE_IN
    return ty


def fill_grids():
    shells = np.full((20, 18, 22), grids.NODE_IN, np.uint8)
    for a, b in ((2, 16), (5, 12)):             # a closed shell and a second one inside it: the space between them stays NODE_IN
        box = shells[a:b, a:b, a:b]
        box[[0, -1]] = grids.NODE_BOUND; box[:, [0, -1]] = grids.NODE_BOUND; box[:, :, [0, -1]] = grids.NODE_BOUND
    bound0 = np.full((9, 7, 13), grids.NODE_IN, np.uint8)
    bound0[0, 0, 0] = grids.NODE_BOUND
    bound0[4, :, :] = grids.NODE_BOUND
    return {"serpentine": serpentine(), "all-in": np.full((10, 9, 66), grids.NODE_IN, np.uint8), "bound-at-origin": bound0, "two-shells": shells}


def line_pass(ty, axis):
    """One directional pass of the device fill (k_geom_fill_z / k_geom_fill_strided): along every line of `axis`, NODE_OUT spreads
    through the NODE_IN cells of its run both ways.  Returns the number of cells turned."""
    t = np.moveaxis(ty, axis, 2)
    wall = (t != grids.NODE_IN) & (t != grids.NODE_OUT)
    run = np.cumsum(wall, axis=2)                            # run id along the line: a wall starts a new one (and holds no fluid itself)
    n_runs = int(run.max()) + 1
    has_out = np.zeros(t.shape[:2] + (n_runs,), bool)
    ii, jj, kk = np.nonzero(t == grids.NODE_OUT)
    has_out[ii, jj, run[ii, jj, kk]] = True
    turn = (t == grids.NODE_IN) & np.take_along_axis(has_out, run, axis=2)
    t[turn] = grids.NODE_OUT
    return int(turn.sum())


def pass_fill(ty):
    """The device algorithm in numpy: seed, then rounds of a Z, a Y and an X pass until a round turns nothing.  -> (grid, rounds)"""
    ty = ty.copy()
    ty[0, 0, 0] = grids.NODE_OUT
    rounds = 0
    while True:
        rounds += 1
        if sum(line_pass(ty, ax) for ax in (2, 1, 0)) == 0:
            return ty, rounds
