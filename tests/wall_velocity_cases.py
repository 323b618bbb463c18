"""Meshes, vertex velocities and expected grids of the Shape3D wall-velocity tests (tests/test_mesh_wall_velocity.py,
tests/test_gpu_mesh_wall_velocity.py).  Expected node arrays come from the twin (shape3d.Shape3D.build with velocities, nodes_of)
alone; the twin's owner is held to an independent painting and its weights to a least-squares projection, both below."""
import copy
import functools

import numpy as np

import mesh_cases as MC
import watertight_cases as W
from cmc_fluid_solver_amd import grids, shape3d

WALL_T = 0.625                     # not 0, not baseT: a wall temperature that went astray shows
GPU_CASES = ["sphere-20", "sphere-320-small", "tetra", "box_pipe_3D", "ragged", "outside", "degenerate"] + list(W.DEGENERATE_ROTATED)
CPU_OWNER_CASES = ["sphere-20", "tetra", "box_pipe_3D", "degenerate"]


def affine(seed=7):
    """a seeded affine velocity field x -> A x + b in grid coordinates: (A [3, 3], b [3])"""
    rng = np.random.default_rng(seed)
    return rng.uniform(-1.0, 1.0, (3, 3)), rng.uniform(-1.0, 1.0, 3)


def velocities(g, seed=7):
    """the affine field of `seed` at the vertices g [n, 3], as the fp32 vertex velocities the loaders hand on"""
    A, b = affine(seed)
    return (np.asarray(g, np.float64) @ A.T + b).astype(np.float32)


def mesh(case):
    """(conservative twin, vertices in grid coordinates, triangles) of a case of watertight_cases.gpu_case"""
    sh, g, idx, _ = W.gpu_case(case)
    return sh, np.asarray(g, np.float32), np.asarray(idx).reshape(-1, 3)


def built(sh, g, idx, vel):
    """a copy of the twin `sh` holding the conservative grid of (g, idx) with owner and, for vel [n, 3], wall_v"""
    sh = copy.copy(sh)
    sh.voxels = "conservative"
    sh.build(g, idx, vel)
    return sh


def nodes_of(sh, wall_T=WALL_T):
    return shape3d.nodes_of(sh, sh.dx, sh.dy, sh.dz, MC.BASE_T, sh.wall_v, wall_T)


@functools.lru_cache(maxsize=None)
def expected(case, reverse=False):
    """(nodes of the twin with the seeded velocities and WALL_T, g, velocities, idx) -- idx reversed on request"""
    sh, g, idx = mesh(case)
    if reverse:
        idx = idx[::-1].copy()
    vel = velocities(g)
    return nodes_of(built(sh, g, idx, vel)), g, vel, idx


def painted_owner(sh, g, idx):
    """The owner by an independent painting: one single-triangle conservative grid per triangle, painted in descending index
    order, so that the smallest index is the last to write a cell.  -1 where no triangle sets the cell."""
    own = np.full((sh.dimx, sh.dimy, sh.dimz), -1, np.int64)
    for t in range(len(idx) - 1, -1, -1):
        one = W.conservative(sh, g, idx[t:t + 1])
        own[one.type == grids.NODE_BOUND] = t
    return own


def projection(p, centre):
    """The orthogonal projection of `centre` onto the plane of the triangle p [3, 3] (float64) by least squares: (point, the
    unclamped barycentric coordinates b0, b1, b2).  Shares nothing with shape3d.wall_weights."""
    E = np.stack([p[1] - p[0], p[2] - p[0]], axis=1)                 # [3, 2]
    sol = np.linalg.lstsq(E, centre - p[0], rcond=None)[0]
    return p[0] + E @ sol, np.array([1.0 - sol[0] - sol[1], sol[0], sol[1]])


# ---- the translating sphere of the physics tests --------------------------------------------------------------------------------

WALL_SPEED = 0.05
RUN_STEPS = 8
RUN_DT = 0.01
RUN_GL = (2, 1)


def translating_grids(speed=WALL_SPEED):
    """The 20-face sphere of W.sphere(20, (15, 19, 15)) scaled 0.7 about its centroid and shifted -3 + 0.5 s cells in x, s = 0 .. 7,
    every vertex at (speed, 0, 0), wallT = baseT: [(nodes of the twin, g, vel, idx)] per step."""
    sh, _ = W.sphere(20, (15, 19, 15))
    g0, idx = sh.subframe(0.0)
    idx = np.asarray(idx).reshape(-1, 3)
    centre = g0.mean(axis=0, dtype=np.float64)
    out = []
    for s in range(RUN_STEPS):
        g = ((g0 - centre) * 0.7 + centre + np.array([-3.0 + 0.5 * s, 0.0, 0.0])).astype(np.float32)
        vel = np.zeros(g.shape, np.float32)
        vel[:, 0] = speed
        out.append((nodes_of(built(sh, g, idx, vel), MC.BASE_T), g, vel, idx))
    return out


def oracle_arrays(nodes, dtype):
    return [np.ascontiguousarray(a, np.uint8) for a in (nodes.type, nodes.bc_vel, nodes.bc_temp)] + \
           [np.ascontiguousarray(v, dtype) for v in (nodes.vx, nodes.vy, nodes.vz, nodes.T)]


def oracle_step(O, o, nodes, dtype, clear):
    """one step of the CPU oracle on the geometry `nodes`: set, CreateSegments, UpdateBoundaries, TimeStep, ClearOutterCells
    -> (status, reported error)"""
    o._f("fs3d_oracle_set_nodes")(o.h, *[O._ptr(x) for x in oracle_arrays(nodes, dtype)])
    o._f("fs3d_oracle_create_segments")(o.h)
    o.update_boundaries()
    rc, err = o.time_step(float(dtype(RUN_DT)), RUN_GL[0], RUN_GL[1], True)
    clear(o, nodes.type == grids.NODE_OUT, MC.BASE_T)
    return rc, err
