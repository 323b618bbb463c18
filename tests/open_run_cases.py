"""Geometries with open fluid runs and with NODE_IN cells on a line's first index, and the CPU oracle's results on them, for
tests/test_open_run_cases.py (CPU conditions) and tests/test_gpu_open_runs.py (the kernels).

Grid3D::GenerateListSegments drops a run of NODE_IN cells that reaches the end of its line without a closing cell: those cells
lie on no segment of that direction, no sweep of it writes them, and the merge that follows averages whatever the sweep's output
layer last held there into temp -- a STALE value (`stale_in_cells` of csrc/fs3d_tables.h).  Which layer is stale where, inside
AdiSolver3D::TimeStep (Z writes next, Y writes half, X writes next):
    X-stale cells read `next` as the Z sweep of the same iteration left it (no initial contents, unless they are Z-stale too);
    Y-stale cells read `half`, which only Y sweeps write: on cells that are Y-stale for good it keeps its initial contents;
    Z-stale cells read `next` as the X sweep of the previous iteration left it (the first iteration: the initial contents).
A case is STALE-SENSITIVE when the oracle's result changes with the initial contents of half / next alone: on those a kernel
that reads the wrong buffer or no value cannot match.  The walk of a line starts at its second cell, so a NODE_IN cell at index
0 becomes the START cell of its segment: a boundary row on a fluid cell that the merge averages as well (`in_starts`).

Every case is a named construction: a base grid and windows of its outer shell set to NODE_IN (`closed=True` leaves them
NODE_BOUND / NODE_VALVE: the closed twin).  What an entry states (stale, in_starts, sensitive) is held to the host table builder
and to the oracle by tests/test_open_run_cases.py.
"""
import collections
import functools

import numpy as np

from cmc_fluid_solver_amd import capi, grids

DT = 0.1
PARAMS = (200.0, 0.72, 1.4)
SENTINEL = 7.25
S = slice
LAYERS = (capi.LAYER_CUR, capi.LAYER_TEMP, capi.LAYER_HALF, capi.LAYER_NEXT)
SEEDS = {capi.LAYER_CUR: 1, capi.LAYER_TEMP: 2, capi.LAYER_HALF: 3, capi.LAYER_NEXT: 4}
ALT_SEEDS = {capi.LAYER_CUR: 1, capi.LAYER_TEMP: 2, capi.LAYER_HALF: 13, capi.LAYER_NEXT: 14}     # other stale contents only

BOX = functools.partial(grids.box, 20, 16, 24, h=0.04)
OBSTACLE = functools.partial(grids.box_with_obstacle, 28, 24, 32, h=0.03)      # the block: i 11..16, j 9..14, k 12..19
WIDE = functools.partial(grids.box, 70, 40, 68, h=0.02)                        # multi-tile X lines, k groups [0,32) [32,64) [64,68)
LONG_Z = functools.partial(grids.box, 12, 14, 70, h=0.02)                      # 70-cell Z lines: the thread-per-line kernel
ODD_Z = functools.partial(grids.box, 20, 16, 33, h=0.04)                       # dimz % 32 == 1 (and % 16): one lane in the last X/Y tile
TALL = functools.partial(grids.box, 90, 93, 68, h=0.015)                       # fp64 Z kernel: one line per wave, 2 rows per group, 93 odd
LONG_Z_PART = functools.partial(grids.box, 12, 10, 132, h=0.01)                # 132-cell Z lines: fp32 one line per wave (33 of 64 lanes), fp64 a pair of waves

# stale: stale_in_cells > 0; in_starts: NODE_IN cells that carry a START row, over the three directions; sensitive: see above;
# part: the sweep directions whose open runs the partition kernels are tested on ("" = none: dims they refuse, or exact-only)
Case = collections.namedtuple("Case", "base windows walls stale in_starts sensitive part why")


def _c(base, windows, stale, in_starts, sensitive, why, part="XYZ", walls=()):
    return Case(base, tuple(windows), tuple(walls), stale, in_starts, sensitive, part, why)


# Windows in the faces i = 0 and i = dimx - 1 are CORNER windows: they run on to the high edges of j and k, so that their cells
# lie on no segment of Y or Z either.  A NODE_IN cell of those two planes that carried an interior row of a Y or Z sweep would
# read its x neighbour one plane outside the arrays -- in the reference and in the CPU oracle alike (a run of the oracle under
# AddressSanitizer on box(20,16,24) with type[-1, 5:9, 6:12] = NODE_IN stops in d_x of DissFuncY, 504 bytes past a field), so
# there is no defined answer to compare with.  Windows in the j and k faces need no such care: index + 1 and index - 1 stay
# inside the flat arrays there (they wrap into the neighbouring row or plane, in the reference as in the kernels).
# tests/test_open_run_cases.py holds every case to this: rows only on cells of the planes 1 .. dimx - 2.
WX, WY, WZ = (S(5, None), S(6, None)), (S(6, 11), S(6, 12)), (S(6, 11), S(5, 9))  # (j, k), (i, k), (i, j) of the small windows
WXO = (S(8, None), S(10, None))                                                   # behind the block of OBSTACLE, as seen along x
CASES = {
    "x_hi": _c(BOX, [(-1,) + WX], True, 0, True, "X runs without a closing cell (the window cells are stale in Y and Z too)"),
    "y_hi": _c(BOX, [(WY[0], -1, WY[1])], True, 0, True, "Y runs without a closing cell: half keeps its first contents there"),
    "z_hi": _c(BOX, [WZ + (-1,)], True, 0, True, "Z runs without a closing cell: next of the previous iteration's X sweep"),
    "x_lo": _c(BOX, [(0,) + WX], True, 170, True, "NODE_IN START rows of X segments (the window cells are stale in Y and Z)"),
    "y_lo": _c(BOX, [(WY[0], 0, WY[1])], False, 30, False, "NODE_IN START rows of Y segments"),
    "z_lo": _c(BOX, [WZ + (0,)], False, 20, False, "NODE_IN START rows of Z segments"),
    "x_through": _c(BOX, [(0,) + WX, (-1,) + WX], True, 0, True, "whole X lines without a segment"),
    "z_through": _c(BOX, [WZ + (0,), WZ + (-1,)], True, 0, True, "whole Z lines without a segment"),
    "x_obstacle_then_open": _c(OBSTACLE, [(-1,) + WXO], True, 0, True,
                               "a closed X segment, its END cell, then a stale tail on the same line"),
    "y_obstacle_then_open": _c(OBSTACLE, [(S(9, 19), -1, S(10, 22))], True, 0, True, "the same along Y"),
    "z_obstacle_then_open": _c(OBSTACLE, [(S(9, 19), S(8, 16), -1)], True, 0, True, "the same along Z"),
    "x_lone_cell": _c(BOX, [(0,) + WX], True, 0, True, "a single stale cell at index 0: the cell after it is a wall",
                      walls=[(1,) + WX]),
    "all_three": _c(OBSTACLE, [(-1,) + WX, (WY[0], -1, WY[1]), (S(17, 22), S(5, 9), -1), WZ + (0,)], True, 20, True,
                    "open high windows in X, Y and Z at once, and a low window in Z (NODE_IN Z START rows) on other lines"),
    # the X/Y partition kernels run the 32 neighbouring k lines of a row as one group
    "part_x_group": _c(WIDE, [(-1, S(10, None), S(32, None))], True, 0, True, "the group k 32..63 is uniform: one shared column, all fluid cells stale", part="X"),
    "part_x_cut": _c(WIDE, [(-1, S(10, None), S(33, None))], True, 0, True, "k 32 stays closed: the group is not uniform", part="X"),
    "part_y_group": _c(WIDE, [(S(10, 14), -1, S(32, 64))], True, 0, True, "the same for the Y kernel", part="Y"),
    "part_y_cut": _c(WIDE, [(S(10, 14), -1, S(33, 64))], True, 0, True, "the same for the Y kernel", part="Y"),
    "part_z_mixed": _c(WIDE, [(S(10, 14), S(9, 21), -1)], True, 0, True, "stale and solved Z lines in the lanes of one wave", part="Z"),
    "z_hi_lone_lane": _c(ODD_Z, [WZ + (-1,)], True, 0, True, "z_hi with dimz = 33: the line's last cell is the only lane of the last X/Y tile, "
                         "and an X / Y row that reads k + 1 (the Z kernels refuse 33-cell lines)", part="XY"),
    "part_y_row_behind": _c(TALL, [(S(10, 14), -1, S(32, 64))], True, 0, True, "fp64 Z kernel, one line per wave-wide access and two rows per "
                            "group: line dimy - 1 opens its group, its j + 1 is the row behind the plane", part="YZ"),
    "part_z_row_behind_132": _c(LONG_Z_PART, [(S(4, 8), -1, S(100, 131))], True, 0, True, "the fp32 twin of part_y_row_behind: Z lines of 132 cells, one per "
                                "wave-wide access; line dimy - 1 is a row of its own, its j + 1 is the row behind the plane", part="Z"),
    "line_fallback": _c(LONG_Z, [(S(4, 8), S(5, 9), -1)], True, 0, True, "Z lines the pipelined kernel refuses: the thread-per-line walk", part=""),
}
EVERY = list(CASES)
ALL = [n for n in EVERY if CASES[n].base not in (TALL, LONG_Z_PART)]   # the exact-kernel matrices leave out the 90x93x68 grid: it is there for
                                                                # one path of the fp64 Z partition kernel and costs as much as the rest together;
                                                                # and its fp32 twin on 132-cell lines, there for the Z partition kernels alone
SENSITIVE = [n for n in EVERY if CASES[n].sensitive]
PART = [n for n in EVERY if CASES[n].part]


def _ro(fields):
    for a in fields:
        a.setflags(write=False)
    return fields


def grid(name, closed=False):
    """The grid of that name (closed: its closed twin); shared, not to be written."""
    return _grid(name, bool(closed))


@functools.lru_cache(maxsize=None)
def _grid(name, closed):
    c = CASES[name]
    g = c.base()
    if not closed:
        for w in c.windows:
            g.type[w] = grids.NODE_IN
    for w in c.walls:
        grids._set_bound(g, w, grids.BC_NOSLIP, grids.BC_NOSLIP, (0.0, 0.0, 0.0), 1.0)
    for a in (g.type, g.bc_vel, g.bc_temp, g.vx, g.vy, g.vz, g.T):
        a.setflags(write=False)
    return g


def window_mask(name):
    m = np.zeros(grid(name).shape, bool)
    for w in CASES[name].windows:
        m[w] = True
    return m


@functools.lru_cache(maxsize=None)
def tables(name):
    """The numpy restatement of the geometry tables of the grid (test_geom_tables.restate); computed once."""
    import test_geom_tables as GT
    return GT.restate(grid(name))


@functools.lru_cache(maxsize=None)
def kinds(name):
    """Row kind per direction, [d][i][j][k], from the restated tables."""
    code = tables(name)["code"].reshape(grid(name).shape)
    return tuple(_ro([(code >> (4 * d)) & 3 for d in range(3)]))


def stale_mask(name, d):
    """NODE_IN cells on no segment of direction d."""
    from geom_rules import ROW_SKIP
    return (grid(name).type == grids.NODE_IN) & (kinds(name)[d] == ROW_SKIP)


def in_start_count(name):
    from geom_rules import ROW_START
    return int(sum(((grid(name).type == grids.NODE_IN) & (k == ROW_START)).sum() for k in kinds(name)))


# ---- the seeded state -------------------------------------------------------------------------------------------------------

def seeded(name, alt=False, closed=False):
    """{layer: fields} for all four layers, in fp32 (an fp64 context or oracle gets the same values); alt: other contents in
    half and next only."""
    return _seeded(name, bool(alt), bool(closed))


@functools.lru_cache(maxsize=8)
def _seeded(name, alt, closed):
    g = grid(name, closed)
    base = [np.ascontiguousarray(a, np.float32) for a in (g.vx, g.vy, g.vz, g.T)]
    return {l: _ro(grids.perturb(base, seed=s)) for l, s in (ALT_SEEDS if alt else SEEDS).items()}


def seed_all(name, s=None, o=None, alt=False, closed=False, sentinel_next=False, x=slice(None)):
    """The same seeded contents in all four layers of a capi.Solver s (planes x of the grid) and of an Oracle o: without it the
    stale values of the first step are whatever the allocation left.  sentinel_next: `next` full of SENTINEL instead."""
    for l, f in seeded(name, alt, closed).items():
        if sentinel_next and l == capi.LAYER_NEXT:
            f = [np.full(a.shape, SENTINEL, np.float32) for a in f]
        if s is not None:
            s.upload_layer(l, [a[x] for a in f])
        if o is not None:
            for v in range(4):
                o.set_field(l, v, f[v].astype(o.dtype))                 # the oracle's layer ids are capi's


def oracle(name, dtype, closed=False):
    from oracle import oracle as O
    assert (O.L_CUR, O.L_TEMP, O.L_HALF, O.L_NEXT) == LAYERS
    return O.Oracle(grid(name, closed), capi.fluid_params(dtype, *PARAMS), dtype)


# ---- the references: computed once, handed out read-only --------------------------------------------------------------------

def merged_sweeps_reference(name, dtype):
    """{d: (next, temp)} after TWO merged sweeps of direction d on the seeded state (every direction starts from it again)."""
    return _merged_sweeps_reference(name, np.dtype(dtype))


@functools.lru_cache(maxsize=4)
def _merged_sweeps_reference(name, dtype):
    o = oracle(name, dtype)
    out = {}
    for d in range(3):
        seed_all(name, o=o)
        for _ in range(2):
            o.sweep(d, DT, capi.LAYER_CUR, capi.LAYER_TEMP, capi.LAYER_NEXT); o.merge(capi.LAYER_NEXT, capi.LAYER_TEMP)
        out[d] = _ro(o.get_layer_fields(capi.LAYER_NEXT)), _ro(o.get_layer_fields(capi.LAYER_TEMP))
    o.close()
    return out


def sentinel_sweep_reference(name, dtype, closed=False):
    """{d: (next, merged temp)} of ONE merged sweep of direction d on the seeded state with `next` full of SENTINEL."""
    return _sentinel_sweep_reference(name, np.dtype(dtype), bool(closed))


@functools.lru_cache(maxsize=8)
def _sentinel_sweep_reference(name, dtype, closed):
    o = oracle(name, dtype, closed)
    out = {}
    for d in range(3):
        seed_all(name, o=o, closed=closed, sentinel_next=True)
        o.sweep(d, DT, capi.LAYER_CUR, capi.LAYER_TEMP, capi.LAYER_NEXT); o.merge(capi.LAYER_NEXT, capi.LAYER_TEMP)
        out[d] = _ro(o.get_layer_fields(capi.LAYER_NEXT)), _ro(o.get_layer_fields(capi.LAYER_TEMP))
    o.close()
    return out


Step = collections.namedtuple("Step", "rc err cur next temp layers")
OUTDIMS = ((0, 0, 0), (7, 6, 5))


def steps_reference(name, dtype, G=4, L=2, steps=3, alt=False, closed=False, get_layers=False):
    """`steps` time steps (UpdateBoundaries + TimeStep) from the seeded state: a Step per step.  get_layers: `layers` are
    GetLayer's (V, T) for OUTDIMS, taken after the fields of every step -- GetLayer stamps the NODE_OUT cells of next with
    99999, which the following steps carry along: for value-for-value comparisons only, a norm over the grid would see little
    else."""
    return _steps_reference(name, np.dtype(dtype), G, L, steps, bool(alt), bool(closed), bool(get_layers))


@functools.lru_cache(maxsize=8)
def _steps_reference(name, dtype, G, L, steps, alt, closed, get_layers):
    o = oracle(name, dtype, closed)
    seed_all(name, o=o, alt=alt, closed=closed)
    out = []
    for _ in range(steps):
        o.update_boundaries()
        rc, e = o.time_step(DT, G, L, True)
        f = [_ro(o.get_layer_fields(l)) for l in (capi.LAYER_CUR, capi.LAYER_NEXT, capi.LAYER_TEMP)]
        out.append(Step(rc, e, *f, [o.get_layer(od) for od in OUTDIMS] if get_layers else None))
    o.close()
    return out
