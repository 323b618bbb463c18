"""Meshes, expected grids and the independent overlap test of the conservative Shape3D voxeliser (tests/test_mesh_watertight.py,
tests/test_gpu_mesh_watertight.py).  Expected grids come from the twin (shape3d.Shape3D(voxels="conservative")) alone; the twin is
held to the float64 separating-axis test below, which shares nothing with its loops."""
import copy
import functools

import numpy as np

import mesh_cases as MC
from test_shape3d import icosphere
from cmc_fluid_solver_amd import grids, shape3d

H = 0.001
SUBDIV = {20: 0, 80: 1, 320: 2, 1280: 3}
SCALES = [0.5 + 0.025 * i for i in range(21)]
# the default rasteriser leaks (no NODE_IN cell at all) at these scales of r = s (30, 38, 30)
LEAKS_320 = [0.7, 0.9]
LEAK_COUNT = {20: 8, 80: 8, 320: 2}
SINGLE = [(20, (15, 19, 15), (28, 35, 28)), (80, (30, 38, 30), (64, 81, 64)), (1280, (57, 72, 57), (120, 151, 120))]


def sphere_text(faces, r):
    """icosphere(1, 0, subdiv) r + (1.5 r + 0.5), millimetres, as the text of a one-frame Shape3D file; and its centre"""
    r = np.array(r, float)
    v, f = icosphere(1, 0, SUBDIV[faces])
    c = 1.5 * r + 0.5
    v = v * r + c
    txt = "1\n%d\n" % len(v) + "".join("%.6g %.6g %.6g 0 0 0\n" % tuple(p) for p in v) + "%d\n" % len(f) + "".join("%d %d %d\n" % tuple(t) for t in f)
    return txt, c


@functools.lru_cache(maxsize=None)
def sphere(faces, r, voxels="conservative"):
    """(Shape3D twin with its grid built, centre cell) of the sphere on h = 0.001 without `align`"""
    txt, c = sphere_text(faces, r)
    sh = shape3d.Shape3D(shape3d.parse_shape3d(txt), H, H, H, False, voxels=voxels)
    cell = tuple(int((p * 1e-3 - o) / H) for p, o in zip(c, sh.bbox[:3]))
    return sh, cell


def closed_report(ty, centre):
    """what a closed shell means, as a dict of counts: NODE_IN cells, the centre and corner cells, NODE_IN cells that touch NODE_OUT"""
    inn, out = ty == grids.NODE_IN, ty == grids.NODE_OUT
    touching = 0
    for ax in range(3):
        a = [slice(None)] * 3; b = [slice(None)] * 3
        a[ax], b[ax] = slice(0, -1), slice(1, None)
        touching += int((inn[tuple(a)] & out[tuple(b)]).sum() + (out[tuple(a)] & inn[tuple(b)]).sum())
    return dict(n_in=int(inn.sum()), centre=int(ty[tuple(centre)]), corner=int(ty[0, 0, 0]), in_touching_out=touching)


def assert_closed(rep):
    assert rep["n_in"] > 0 and rep["centre"] == grids.NODE_IN and rep["corner"] == grids.NODE_OUT and rep["in_touching_out"] == 0, rep


def conservative(sh, g, idx):
    """a copy of the twin `sh` holding the conservative grid of the mesh (g, idx)"""
    sh = copy.copy(sh)
    sh.voxels = "conservative"
    sh.build(g, idx)
    return sh


def blank(dims):
    """a twin without frames: dims only, for build() on meshes given in grid coordinates"""
    sh = shape3d.Shape3D.__new__(shape3d.Shape3D)
    sh.voxels = "conservative"
    sh.dimx, sh.dimy, sh.dimz = dims
    sh.dx = sh.dy = sh.dz = H
    return sh


# ---- the independent restatement ------------------------------------------------------------------------------------------------

def sat_overlap(dims, g, idx, grow):
    """float64, whole arrays: the cells whose unit box, grown by `grow` on every side, is not separated from some triangle by any
    of the 13 axes (3 of the box, the normal, 9 edge x axis) -- touching counts as overlap.  Every triangle against every cell
    around its bounding box."""
    hit = np.zeros(dims, bool)
    h = 0.5 + grow
    eye = np.eye(3)
    for t in np.asarray(idx):
        v = np.asarray(g, np.float64)[t]
        lo = np.maximum(np.floor(v.min(0)).astype(int) - 2, 0); hi = np.minimum(np.ceil(v.max(0)).astype(int) + 2, np.array(dims))
        if (lo >= hi).any():
            continue
        c = np.stack(np.meshgrid(*[np.arange(a, b) + 0.5 for a, b in zip(lo, hi)], indexing="ij"), -1).reshape(-1, 3)
        e = [v[1] - v[0], v[2] - v[1], v[0] - v[2]]
        axes = list(eye) + [np.cross(e[0], e[1])] + [np.cross(ee, ax) for ee in e for ax in eye]
        sep = np.zeros(len(c), bool)
        for a in axes:
            p = (v @ a)[None, :] - (c @ a)[:, None]
            r = h * np.abs(a).sum()
            sep |= (p.min(1) > r) | (p.max(1) < -r)
        hit[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] |= (~sep).reshape(hi - lo)
    return hit


def tolerance(g, idx):
    """slack + rounding bound of the twin for the mesh: VOXEL_TOL * L, L = the largest local coordinate of any triangle + 2
    (a triangle's local vertices lie within its extent + 1 of the origin)"""
    tri = np.asarray(g, np.float64)[np.asarray(idx)]
    return shape3d.VOXEL_TOL * ((tri.max(1) - tri.min(1)).max() + 3)


def restatement(sh, g, idx):
    """(shell cells, must-be-set cells missing, set cells that must not be, free cells) of the conservative twin grid `sh` against
    the float64 test.  Must be set: float64 finds the closed box overlapping or touching (margin >= 0 as computed).  Nothing is
    taken off this side: the rule is the closed box, rounding may only add cells, and the twin's slack (at least 2^-33 of a
    cell, 1e-10) exceeds this test's own noise (below 1e-12 at these coordinates), so a cell float64 misjudges by its noise is set either way.
    This is what makes a face ON a cell plane (box_pipe_3D: margin exactly zero on both sides) a checked case and not a free
    one.  Must not be set: separated by more than the tolerance.  Between the two a cell is free."""
    tol = tolerance(g, idx)
    must = sat_overlap(sh.type.shape, g, idx, 0.0)
    may = sat_overlap(sh.type.shape, g, idx, tol)
    b = sh.type == grids.NODE_BOUND
    # NODE_BOUND only ever comes from the voxeliser (the fill turns NODE_IN into NODE_OUT)
    return int(b.sum()), int((must & ~b).sum()), int((b & ~may).sum()), int((may & ~must).sum())


# ---- meshes in grid coordinates -----------------------------------------------------------------------------------------------

DEGENERATE = {   # one triangle each on a 16 x 12 x 10 grid; the longest edge is (first, last) of `seg`
    "repeated-vertex": ([[1.25, 2.5, 3.75], [9.5, 7.25, 6.5], [1.25, 2.5, 3.75]], ([1.25, 2.5, 3.75], [9.5, 7.25, 6.5])),
    "zero-length-edge": ([[2.5, 1.5, 8.25], [2.5, 1.5, 8.25], [12.75, 9.5, 1.5]], ([2.5, 1.5, 8.25], [12.75, 9.5, 1.5])),
    "collinear": ([[1.25, 1.5, 1.75], [5.25, 3.5, 2.75], [13.25, 7.5, 4.75]], ([1.25, 1.5, 1.75], [13.25, 7.5, 4.75])),
    "point": ([[4.5, 4.25, 4.75]] * 3, ([4.5, 4.25, 4.75], [4.5, 4.25, 4.75])),
    "on-cell-planes": ([[3.0, 2.0, 5.0], [3.0, 9.0, 5.0], [3.0, 5.0, 5.0]], ([3.0, 2.0, 5.0], [3.0, 9.0, 5.0])),
}
DEGENERATE_DIMS = (16, 12, 10)


def degenerate_mesh():
    """all of DEGENERATE as one mesh, and a needle below the degenerate threshold"""
    g = np.array([p for tri, _ in DEGENERATE.values() for p in tri] + [[2.0, 10.5, 8.5], [14.5, 10.5, 8.5], [8.0, 10.5 + 2.0 ** -18, 8.5]], np.float32)
    return g, np.arange(len(g)).reshape(-1, 3)


# The degenerate mesh with its coordinates and its grid rotated: (x, y, z) -> (y, z, x) and (z, x, y).  Every triangle of DEGENERATE,
# and the needle, has its smallest extent along z, or ties and takes x; rotated, the depth axis of a degenerate triangle is y as well.
DEGENERATE_ROTATED = {"degenerate-yzx": (1, 2, 0), "degenerate-zxy": (2, 0, 1)}


@functools.lru_cache(maxsize=None)
def gpu_case(case):
    """(conservative twin, vertices in grid coordinates, triangles, centre cell or None) of a case of tests/test_gpu_mesh_watertight.py"""
    spheres = {"sphere-20": (20, (15, 19, 15)), "sphere-80": (80, (30, 38, 30)), "sphere-320-small": (320, (9, 11, 9))}
    if case in spheres:
        sh, cell = sphere(*spheres[case])
        g, idx = sh.subframe(0.0)
        return sh, g, idx, cell
    if case == "degenerate":
        sh = blank(DEGENERATE_DIMS)
        g, idx = degenerate_mesh()
        sh.build(g, idx)
        return sh, g, idx, None
    if case in DEGENERATE_ROTATED:
        perm = list(DEGENERATE_ROTATED[case])
        sh = blank(tuple(DEGENERATE_DIMS[c] for c in perm))
        g, idx = degenerate_mesh()
        g = np.ascontiguousarray(g[:, perm])
        sh.build(g, idx)
        return sh, g, idx, None
    sh, g, idx, _ = MC.load_case({"ragged": "sphere-ragged", "outside": "sphere-outside"}.get(case, case))
    return conservative(sh, g, idx), g, idx, None


GPU_CASES = ["sphere-20", "sphere-80", "sphere-320-small", "box_pipe_3D", "tetra", "ragged", "outside", "degenerate"] + list(DEGENERATE_ROTATED)
