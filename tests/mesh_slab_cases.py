"""Meshes and expected grids of the Shape3D slab tests (tests/test_mesh_slab_api.py, tests/test_gpu_mesh_slab.py): a slab context
that started from a box and was given a mesh through fs3d_update_nodes_shape3d_slab / _vel_slab is held to a fresh slab context
that uploaded the twin's nodes of the GLOBAL grid.  Expected nodes come from cmc_fluid_solver_amd/shape3d.py alone, through the
case modules of the single-context mesh tests.  Every case is shared and read-only.

    sphere-t2       reference rasteriser, 32^3 (dimz % 4 == 0: four cells per thread).  With four ranks the last slab holds
                    neither a wall nor a fluid cell.
    sphere-ragged   reference rasteriser, 25 x 24 x 25 (dimz % 4 != 0: cell by cell).
    sphere-80-vel   conservative, the second geometry of test_update_with_velocities_equals_upload_of_the_twin: the 80-face sphere
                    scaled by 0.9 and shifted by 3 on 64 x 81 x 64, vertex velocities wall_velocity_cases.velocities(g) 2^-10,
                    wallT = wall_velocity_cases.WALL_T.  Every slab of 2, 3 and 4 ranks holds NODE_IN cells and moving wall cells.
    sphere-80-zero  the same mesh with zero velocities and wallT = 0: the nodes of the plain entry.
    tube-cube       conservative, 24 x 16 x 16, 3 ranks of 8 planes: an open-ended square tube along x through all three slabs
                    and a closed cube inside the middle one.  The tube's inside is NODE_OUT (the fill enters through its ends, in
                    the outer slabs); a fill that stopped at the middle slab's cuts would leave it NODE_IN there.
"""
import functools

import numpy as np

import mesh_cases as MC
import wall_velocity_cases as WV
import watertight_cases as W
from cmc_fluid_solver_amd import grids
from cmc_fluid_solver_amd.slab import slab_range

TABLE_CASES = ["sphere-t2", "sphere-ragged", "sphere-80-vel", "tube-cube"]
RANKS = {"sphere-t2": (2, 3, 4), "sphere-ragged": (2, 3, 4), "sphere-80-vel": (2, 3, 4), "sphere-80-zero": (2, 3, 4), "tube-cube": (3,)}
TUBE_DIMS = (24, 16, 16)
TUBE_SLAB = (8, 16)                 # the middle one of 3 ranks


class Case:
    """want: the twin's nodes of the global grid; g, idx: the mesh in global grid coordinates; vel / wallT: None for the plain
    entry; voxels: the FS3D_OPT_MESH_VOXELS word of capi."""
    def __init__(self, want, g, idx, voxels, vel=None, wallT=None):
        self.want, self.g, self.idx, self.voxels, self.vel, self.wallT = want, g, idx, voxels, vel, wallT
        for a in (want.type, want.bc_vel, want.bc_temp, want.vx, want.vy, want.vz, want.T, self.g) + (() if vel is None else (vel,)):
            a.setflags(write=False)

    def start(self):
        """the box of the case's dims a context starts from"""
        b = grids.box(*self.want.shape)
        b.dx, b.dy, b.dz = self.want.dx, self.want.dy, self.want.dz
        return b

    def update(self, s):
        """the case's mesh through the slab entry it is about -> n_seg"""
        if self.vel is None:
            return s.update_nodes_shape3d_slab(self.g, self.idx, MC.BASE_T, voxels=self.voxels)
        return s.update_nodes_shape3d_vel_slab(self.g, self.vel, self.idx, MC.BASE_T, self.wallT, voxels=self.voxels)


def tube_cube_mesh():
    """(vertices [16, 3] in grid coordinates, triangles [20, 3]): the tube's four sides (8 triangles), then the cube (12)"""
    ring = [(3.5, 3.5), (12.5, 3.5), (12.5, 12.5), (3.5, 12.5)]
    v = [(x, y, z) for x in (4.5, 19.5) for y, z in ring]
    tri = []
    for q in range(4):
        q1 = (q + 1) % 4
        tri += [(q, 4 + q, 4 + q1), (q, 4 + q1, q1)]
    lo, hi = (10.5, 6.5, 6.5), (13.5, 9.5, 9.5)
    c0 = len(v)
    v += [(x, y, z) for x in (lo[0], hi[0]) for y in (lo[1], hi[1]) for z in (lo[2], hi[2])]          # index c0 + 4 i + 2 j + k
    for ax in range(3):
        b, c = [a for a in range(3) if a != ax]
        for side in (0, 1):
            def at(sb, sc):
                bit = [0, 0, 0]
                bit[ax], bit[b], bit[c] = side, sb, sc
                return c0 + 4 * bit[0] + 2 * bit[1] + bit[2]
            tri += [(at(0, 0), at(1, 0), at(1, 1)), (at(0, 0), at(1, 1), at(0, 1))]
    return np.array(v, np.float32), np.array(tri)


def sphere80():
    """(twin, vertices, triangles, velocities) of the second geometry of test_update_with_velocities_equals_upload_of_the_twin"""
    sh, _ = W.sphere(80, (30, 38, 30))
    g = (sh.subframe(0.0)[0] * np.float32(0.9) + np.float32(3.0)).astype(np.float32)
    idx = np.asarray(sh.subframe(0.0)[1]).reshape(-1, 3)
    vel = (WV.velocities(g) * np.float32(2.0 ** -10)).astype(np.float32)
    return sh, g, idx, vel


@functools.lru_cache(maxsize=None)
def case(name):
    if name in ("sphere-t2", "sphere-ragged"):
        sh, g, idx, _ = MC.load_case(name)
        return Case(MC.nodes_of(sh), np.array(g, np.float32), np.asarray(idx).reshape(-1, 3), "reference")
    if name == "sphere-80-vel":
        sh, g, idx, vel = sphere80()
        return Case(WV.nodes_of(WV.built(sh, g, idx, vel)), g, idx, "conservative", vel, WV.WALL_T)
    if name == "sphere-80-zero":
        sh, g, idx, vel = sphere80()
        return Case(MC.nodes_of(W.conservative(sh, g, idx)), g, idx, "conservative", np.zeros_like(vel), 0.0)
    assert name == "tube-cube"
    g, idx = tube_cube_mesh()
    sh = W.blank(TUBE_DIMS)
    sh.build(g, idx)
    return Case(MC.nodes_of(sh), g, idx, "conservative")


def ranges(dimx, nranks):
    return [slab_range(dimx, r, nranks) for r in range(nranks)]


def slab_local_fill(ty, xr):
    """The type array of the planes xr if the fill ran on them alone, seeded at the slab's own corner: what the global fill must NOT give."""
    pre = np.where(ty[xr[0]:xr[1]] == grids.NODE_OUT, grids.NODE_IN, ty[xr[0]:xr[1]]).astype(np.uint8)      # NODE_OUT comes from the fill alone
    return MC.label_fill(pre)
