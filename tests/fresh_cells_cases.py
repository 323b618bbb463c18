"""Geometry pairs and seeded fields of the fresh-cell tests (tests/test_fresh_cells_cases.py, tests/test_gpu_fresh_cells.py).
A case is (nodes before the update, nodes after it); the expected fields come from the twin
cmc_fluid_solver_amd.fresh_cells.fill_fresh_cells alone.  Two grids: 12 x 10 x 16 (1920 cells, a multiple of 8: the classifying
kernel's 8-cell path throughout) and 9 x 7 x 11 (693 = 86 * 8 + 5 cells, every dim odd: its last cells go one by one).
Walls inside the box are NOSLIP / NOSLIP, so that a wall one cell thick between two fluid runs is a geometry the upload takes."""
import functools

import numpy as np

from cmc_fluid_solver_amd import fresh_cells, grids

SIZES = {"12x10x16": (12, 10, 16), "9x7x11": (9, 7, 11)}
CASES = ["one-layer-x", "one-layer-y", "one-layer-z", "thick-both", "thick-one", "pocket", "none", "faces", "capped", "mixed-origin"]
MAX_ROUNDS = {"capped": 2}
# rounds the twin must report (a wall slab of thickness t: ceil(t / 2) with fluid on both sides, t with fluid on one)
ROUNDS = {"one-layer-x": 1, "one-layer-y": 1, "one-layer-z": 1, "thick-both": 3, "thick-one": 5, "none": 0, "capped": 2}
LEAVES_SOME = ("pocket", "capped")                       # cases with fresh cells no round reaches


def _wall(n, sel):
    grids._set_bound(n, sel, grids.BC_NOSLIP, grids.BC_NOSLIP, (0.0, 0.0, 0.0), 0.5)


def _fluid(n, sel):
    n.type[sel] = grids.NODE_IN
    n.bc_vel[sel] = grids.BC_NOSLIP
    n.bc_temp[sel] = grids.BC_NOSLIP
    n.vx[sel] = n.vy[sel] = n.vz[sel] = 0.0
    n.T[sel] = 1.0


def _plane(axis, p):
    """the interior cells of plane `p` along `axis`"""
    sel = [slice(1, -1)] * 3
    sel[axis] = p
    return tuple(sel)


def _slab(lo, hi):
    return (slice(lo, hi + 1), slice(1, -1), slice(1, -1))


BLOCK = (slice(2, 7), slice(2, 5), slice(2, 9))          # i 2..6, j 2..4, k 2..8: fits both grids
INNER = (slice(3, 6), slice(3, 4), slice(3, 8))          # its inside


@functools.lru_cache(maxsize=None)
def pair(name, size):
    """(nodes of the geometry before the update, nodes of the one after it)"""
    dims = SIZES[size]
    a, b = grids.box(*dims), grids.box(*dims)
    if name.startswith("one-layer-"):
        axis = "xyz".index(name[-1])
        p = dims[axis] // 2
        _wall(a, _plane(axis, p)); _wall(b, _plane(axis, p + 1))
    elif name == "thick-both":
        _wall(a, _slab(2, 6))                            # fluid at i = 1 and from i = 7 on
    elif name in ("thick-one", "capped"):
        _wall(a, _slab(1, 5))                            # against the shell at i = 0: fluid from i = 6 on only
    elif name == "pocket":
        _wall(a, BLOCK)
        _wall(b, (slice(3, 7),) + BLOCK[1:])             # the block loses its plane i = 2 (filled) ...
        _fluid(b, (slice(4, 6),) + INNER[1:])            # ... and is hollow: fresh cells behind walls on all sides
    elif name == "none":
        a, b = grids.box_with_obstacle(*dims), grids.box_with_obstacle(*dims)
    elif name == "faces":
        # NODE_IN on all six faces: the corner (0, 0, 0) with its three edges, the opposite corner, a window in every face
        nx, ny, nz = dims
        for sel in ((slice(0, 2), slice(0, 3), slice(0, 3)), (slice(nx - 2, nx), slice(ny - 3, ny), slice(nz - 3, nz)),
                    (0, slice(4, 6), slice(5, 8)), (nx - 1, slice(4, 6), slice(5, 8)), (slice(4, 7), 0, slice(5, 8)),
                    (slice(4, 7), ny - 1, slice(5, 8)), (slice(4, 7), slice(4, 6), 0), (slice(4, 7), slice(4, 6), nz - 1)):
            _fluid(b, sel)
    elif name == "mixed-origin":
        _wall(a, BLOCK)                                  # BOUND ...
        a.type[INNER] = grids.NODE_OUT                   # ... around OUT; the block goes
        _fluid(b, (0, slice(2, 4), slice(2, 5)))         # and a piece of the inflow VALVE turns fluid
    else:
        raise KeyError(name)
    return a, b


def fields(size, dtype, seed):
    """four different seeded fields over ALL cells (walls and outside too: the fill must not touch them)"""
    rng = np.random.default_rng(seed)
    return [np.ascontiguousarray(rng.uniform(-1.0, 1.0, SIZES[size]) + off, dtype) for off in (0.0, 0.25, -0.5, 1.0)]


@functools.lru_cache(maxsize=None)
def expected(name, size, dtype, seed):
    """(filled fields, info) of the twin; read-only"""
    a, b = pair(name, size)
    out, info = fresh_cells.fill_fresh_cells(a.type, b.type, fields(size, dtype, seed), MAX_ROUNDS.get(name, 0))
    for f in out:
        f.setflags(write=False)
    return out, info
