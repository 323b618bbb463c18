"""Expected grids and the independent restatement of the thin Shape3D shell (voxels="conservative", shell="cross":
tests/test_mesh_thin_shell.py, tests/test_gpu_mesh_thin_shell.py).  Meshes are those of tests/watertight_cases.py; expected grids come
from the twin (shape3d.Shape3D(..., shell="cross")) alone; the twin is held to the float64 separating-axis test below, which shares
nothing with its loops."""
import copy
import functools

import numpy as np

import mesh_cases as MC
import wall_velocity_cases as WV
import watertight_cases as W
from cmc_fluid_solver_amd import grids, shape3d

# NODE_BOUND and NODE_IN cells of the cases of W.gpu_case: (conservative, thin).  box_pipe_3D: its faces lie on cell planes, both
# neighbours touch, the fluid is unchanged; degenerate triangles keep the conservative treatment (that grid has no NODE_IN cell).
PINS = {
    "sphere-20": ((3718, 2052), (9090, 9836)),
    "sphere-80": ((18454, 10198), (116124, 119999)),
    "sphere-320-small": ((1734, 957), (2809, 3168)),
    "tetra": ((15135, 6747), (10053, 13423)),
    "ragged": ((2094, 1174), (3891, 4322)),
    "outside": ((646, 367), (1361, 1490)),
    "box_pipe_3D": ((120016, 118808), (941192, 941192)),
    "degenerate": ((114, 114), None),
    "degenerate-yzx": ((114, 114), None),
    "degenerate-zxy": ((114, 114), None),
}
RESTATED = ["sphere-20", "tetra", "outside", "sphere-320-small", "box_pipe_3D"]


def thin(sh, g, idx, vel=None):
    """a copy of the twin `sh` holding the thin grid of the mesh (g, idx) (with vertex velocities: owner and wall_v as well)"""
    sh = copy.copy(sh)
    sh.voxels, sh.shell = "conservative", "cross"
    sh.build(g, idx, vel)
    return sh


@functools.lru_cache(maxsize=None)
def sphere(faces, r):
    """(thin twin, conservative twin, centre cell) of W.sphere(faces, r)"""
    sh, cell = W.sphere(faces, r)
    return thin(sh, *sh.subframe(0.0)), sh, cell


@functools.lru_cache(maxsize=None)
def gpu_case(case):
    """(thin twin, conservative twin, vertices in grid coordinates, triangles, centre cell or None) of a case of W.gpu_case"""
    sh, g, idx, cell = W.gpu_case(case)
    return thin(sh, g, idx), sh, g, idx, cell


def counts(sh):
    return int((sh.type == grids.NODE_BOUND).sum()), int((sh.type == grids.NODE_IN).sum())


def nodes_of(sh):
    return shape3d.nodes_of(sh, sh.dx, sh.dy, sh.dz, MC.BASE_T)


# ---- the independent restatement ------------------------------------------------------------------------------------------------

def sat_overlap_boxes(dims, v, lo, hi, half):
    """float64: of the cells lo .. hi, those whose box of per-axis half-extents `half` about the cell's centre is not separated from
    the triangle v [3, 3] by any of 16 axes -- the 3 of the box, the normal, the 9 edge x axis, and the 3 normal x axis (the
    in-plane normals of a box that has shrunk to a segment: without them a segment in the triangle's plane that passes beside it is
    not told apart).  Touching counts as overlap.  Separating axes of a convex pair: any axis that separates proves disjointness,
    and for a triangle against a box or a segment these are complete."""
    eye = np.eye(3)
    c = np.stack(np.meshgrid(*[np.arange(a, b) + 0.5 for a, b in zip(lo, hi)], indexing="ij"), -1).reshape(-1, 3)
    e = [v[1] - v[0], v[2] - v[1], v[0] - v[2]]
    n = np.cross(e[0], e[1])
    axes = list(eye) + [n] + [np.cross(ee, ax) for ee in e for ax in eye] + [np.cross(n, ax) for ax in eye]
    sep = np.zeros(len(c), bool)
    for a in axes:
        p = (v @ a)[None, :] - (c @ a)[:, None]
        r = float((np.asarray(half) * np.abs(a)).sum())
        sep |= (p.min(1) > r) | (p.max(1) < -r)
    return (~sep).reshape(hi - lo)


def cross_overlap(dims, g, idx, grow):
    """The thin rule, per triangle: a cell is hit iff its unit box overlaps the triangle and one of its three centre segments --
    half-extents (1/2, 0, 0), (0, 1/2, 0), (0, 0, 1/2) -- does, every half-extent grown by `grow`.  A triangle below the twin's area
    threshold keeps the box test alone."""
    hit = np.zeros(dims, bool)
    for t in np.asarray(idx):
        v = np.asarray(g, np.float64)[t]
        lo = np.maximum(np.floor(v.min(0)).astype(int) - 2, 0); hi = np.minimum(np.ceil(v.max(0)).astype(int) + 2, np.array(dims))
        if (lo >= hi).any():
            continue
        m = sat_overlap_boxes(dims, v, lo, hi, np.full(3, 0.5 + grow))
        n = np.cross(v[1] - v[0], v[2] - v[0])
        if n @ n >= shape3d.VOXEL_DEGENERATE:
            seg = np.zeros(m.shape, bool)
            for ax in range(3):
                half = np.full(3, grow)
                half[ax] += 0.5
                seg |= sat_overlap_boxes(dims, v, lo, hi, half)
            m &= seg
        hit[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] |= m
    return hit


def restatement(sh, g, idx):
    """(shell cells, must-be-set cells missing, set cells that must not be, free cells) of the thin twin grid `sh` against the
    float64 test, as W.restatement holds the conservative grid: must = the rule as float64 computes it (touching counts), may = the
    same grown by the twin's slack + rounding bound W.tolerance; between the two a cell is free."""
    tol = W.tolerance(g, idx)
    must = cross_overlap(sh.type.shape, g, idx, 0.0)
    may = cross_overlap(sh.type.shape, g, idx, tol)
    b = sh.type == grids.NODE_BOUND
    return int(b.sum()), int((must & ~b).sum()), int((b & ~may).sum()), int((may & ~must).sum())


# ---- wall velocities: the translating sphere of wall_velocity_cases with the thin shell -------------------------------------------

@functools.lru_cache(maxsize=None)
def translating_grids():
    """[(thin nodes, conservative nodes, g, vel, idx, thin owner, conservative owner)] per step of WV.translating_grids"""
    sh, _ = W.sphere(20, (15, 19, 15))
    out = []
    for nodes, g, vel, idx in WV.translating_grids():
        t, c = thin(sh, g, idx, vel), WV.built(sh, g, idx, vel)
        out.append((WV.nodes_of(t, MC.BASE_T), nodes, g, vel, idx, t.owner, c.owner))
    return out
