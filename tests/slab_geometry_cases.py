"""Geometry pairs A -> B for tests/test_gpu_slab_geometry.py: a slab context that uploaded A and was given B through
fs3d_update_nodes_slab is held to a fresh slab context that uploaded B.  Every grid is shared and read-only.

    obstacle     grids.box_with_obstacle(30, 24, 32): the block (planes 12..18) moved one plane in x, to 13..19.  30 planes cut
                 into 2, 3 and 4 slabs at 15 | 10, 20 | 8, 16, 23: the block lies across the cuts 15 and 16, and with 3 slabs its
                 last wall plane is the last plane of slab 1 -- the cell that closes one X segment and opens the next sits on
                 one side of the cut, the fluid it opens on the other.  4 slabs are uneven (8, 8, 7, 7).
    obstacle2    the same moved two planes (14..20): across the cut at 20 as well.
    solid_from   a box of 16 x 12 x 40 (two groups of 32 k, the second ragged: 8 lines) in which everything from plane p on is
                 solid: plane p a wall, the planes behind it NODE_OUT.  With p = the first plane of slab 1 the piece of every X line
                 in slab 1 holds the line's END cell and no NODE_IN cell: live by the definition of the tables ("no cell on a segment
                 and none NODE_IN"), dead by the shortcut "no NODE_IN cell" that holds for whole lines only.  p depends on the
                 number of ranks.
    open runs    x_obstacle_then_open, x_through, all_three of tests/open_run_cases.py, from their closed twins: stale cells, X
                 lines without a closing cell, NODE_IN START rows.
    dimz18       box(16, 14, 18) -> box_with_obstacle(16, 14, 18): dimz % 4 != 0.
"""
import functools

import numpy as np

import open_run_cases as ORC
from cmc_fluid_solver_amd import grids
from cmc_fluid_solver_amd.slab import slab_range

BASE_T = 1.0
OPEN = ("x_obstacle_then_open", "x_through", "all_three")
TABLE_PAIRS = ["obstacle", "obstacle2", "solid_from", "dimz18"] + list(OPEN)     # test 1
STEP_PAIRS = ["obstacle"] + list(OPEN)                                             # test 3: pairs a and c
AUTO_PAIRS = ["obstacle", "solid_from"]                                            # test 4: pairs a and b


def _freeze(g):
    for a in (g.type, g.bc_vel, g.bc_temp, g.vx, g.vy, g.vz, g.T):
        a.setflags(write=False)
    return g


def _obstacle(shift):
    """grids.box_with_obstacle(30, 24, 32, h=0.03) with its block `shift` planes further along x."""
    n = grids.box(30, 24, 32, h=0.03)
    r = [(max(2, int(0.4 * d)), min(d - 3, int(0.6 * d))) for d in n.shape]
    r[0] = (r[0][0] + shift, r[0][1] + shift)
    assert r[0][1] <= n.dimx - 3
    blk = np.zeros(n.shape, bool)
    blk[r[0][0]:r[0][1] + 1, r[1][0]:r[1][1] + 1, r[2][0]:r[2][1] + 1] = True
    inner = np.zeros(n.shape, bool)
    inner[r[0][0] + 1:r[0][1], r[1][0] + 1:r[1][1], r[2][0] + 1:r[2][1]] = True
    grids._set_bound(n, blk, grids.BC_NOSLIP, grids.BC_FREE, (0.0, 0.0, 0.0), BASE_T)
    n.type[inner] = grids.NODE_OUT
    n.bc_vel[inner] = grids.BC_NOSLIP
    n.bc_temp[inner] = grids.BC_NOSLIP
    n.T[inner] = 0.0
    return n


def _solid_from(p):
    n = grids.box(16, 12, 40)
    grids._set_bound(n, np.s_[p:], grids.BC_NOSLIP, grids.BC_FREE, (0.0, 0.0, 0.0), BASE_T)
    n.type[p + 1:] = grids.NODE_OUT
    return n


@functools.lru_cache(maxsize=None)
def pair(name, nranks=2):
    """(A, B); nranks matters for solid_from only."""
    if name == "obstacle":
        assert np.array_equal(_obstacle(0).type, grids.box_with_obstacle(30, 24, 32, h=0.03).type)
        return _freeze(grids.box_with_obstacle(30, 24, 32, h=0.03)), _freeze(_obstacle(1))
    if name == "obstacle2":
        return _freeze(grids.box_with_obstacle(30, 24, 32, h=0.03)), _freeze(_obstacle(2))
    if name == "solid_from":
        return _freeze(grids.box(16, 12, 40)), _freeze(_solid_from(slab_range(16, 1, nranks)[0]))
    if name == "dimz18":
        return _freeze(grids.box(16, 14, 18)), _freeze(grids.box_with_obstacle(16, 14, 18))
    assert name in OPEN
    return ORC.grid(name, closed=True), ORC.grid(name)


def ranges(dimx, nranks):
    return [slab_range(dimx, r, nranks) for r in range(nranks)]


# ---- refusals ------------------------------------------------------------------------------------------------------------------
REFUSAL_DIMS = (12, 12, 12)          # 3 ranks: planes 0..3, 4..7, 8..11


def baffle_x():
    """A FREE baffle one cell thick across X lines, in plane 2 (rank 0 of 3): the cell closes one X segment and opens the next.
    The X lines are global: every rank's tables are refused."""
    g = grids.box(*REFUSAL_DIMS)
    g.type[2, 4:8, 4:8] = grids.NODE_BOUND
    g.bc_temp[2, 4:8, 4:8] = grids.BC_FREE
    return _freeze(g)


def baffle_y():
    """The same across Y lines, two planes thick in x (so no X line sees a shared cell) in the planes 5, 6 (rank 1 of 3): only the
    tables of rank 1 are refused."""
    g = grids.box(*REFUSAL_DIMS)
    g.type[5:7, 6, 4:8] = grids.NODE_BOUND
    g.bc_temp[5:7, 6, 4:8] = grids.BC_FREE
    return _freeze(g)
