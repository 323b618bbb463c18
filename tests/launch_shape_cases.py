"""One small grid per launch shape of the partition sweep kernels (csrc/kernels_part.hip), with the launch record each must
produce, for tests/test_launch_shape_cases.py (CPU conditions) and tests/test_gpu_launch_shapes.py (the kernels).

The host dispatch picks a template instance and launch parameters from the grid's dimensions alone:
    X/Y  k_sweep_part<R, DIR, M, NCH, LT, XB>, `order`       part_dispatch_xy, part_dispatch_xslab, part_launch_xy
    Z    k_sweep_part_z<R, LPL, NW>, LG rows per wave        part_dispatch_z, part_launch_z
fs3d_last_sweep_launch reports what was launched, so an entry whose grid no longer reaches its instance after a dispatch threshold
moves fails by name instead of testing something else.  A record is the C array without its trailing zeros:
    X/Y  (1, M, NCH, LT, XB, order, workgroups)              Z  (2, LPL, NW, LG, n_grp, workgroups)

Every new grid is a bc_cases.plates grid with the face assignment B -- both end rows of every direction FREE in velocity or in
temperature, the only end rows that couple to their neighbour -- and an FF plate whose END row sits on the last cell of a `unit`
(an X/Y chunk, a Z lane, the lower wave of a pair, a slab) and whose START row on the first cell of the next.  The plates of the
two other axes lie on cells 2, 3.  The existing bc_cases grids that already hold a shape are named too, for their records.

The references (the CPU oracle in fp32 and in fp64 on the same seeded state, one sweep of the entry's direction) are computed once
per process and handed out read-only, as in bc_cases.
"""
import collections
import functools

import numpy as np

import bc_cases as BC
from cmc_fluid_solver_amd import capi, grids

# grid: a name of bc_cases.GRIDS, or None: plates(dims, h, B, FF, pos).  d: the sweep direction.  unit: see above (None with a
# bc_cases grid, whose edges tests/test_bc_cases.py holds).  record: pass 0; record1: the interface pass of a slab's X sweep.
# fuses: the FS3D_OPT_FUSE_MERGE values the GPU test runs.
Case = collections.namedtuple("Case", "name grid dims h dtype d ranks pos unit record record1 fuses why")
F32, F64 = np.float32, np.float64
CASES = collections.OrderedDict()


def _h(dims):
    """The cell size: 0.004 to 300 cells in the longest line, 0.003 to 400, 0.002 beyond.  Small on short lines too: a chunk's or a
    lane's interface row couples to the next one with (vis / b)-like decay over the chunk, 0.73^16 = 6e-3 at h = 0.004 and
    0.86^16 = 9e-2 at 0.002 but 0.47^16 = 6e-6 at 0.01 and 1e-14 at 0.03 (the bc_cases grids), where a wrong interface solve would
    be lost in the rounding."""
    n = max(dims)
    return 0.004 if n <= 300 else 0.003 if n <= 400 else 0.002


def _c(name, dims, d, edge, unit, record, why, dtype=F32, ranks=1, record1=None, fuses=(1,)):
    pos = [2, 2, 2]
    pos[d] = edge
    assert name not in CASES
    CASES[name] = Case(name, None, tuple(dims), _h(dims), dtype, d, ranks, tuple(pos), unit, tuple(record), record1 and tuple(record1), fuses, why)


def _bc(name, grid, d, record, why, dtype=F32, ranks=1, record1=None):
    dims, h = BC.GRIDS[grid].args[:2]
    assert name not in CASES
    CASES[name] = Case(name, grid, tuple(dims), h, dtype, d, ranks, None, None, tuple(record), record1 and tuple(record1), (1,), why)


X, Y, Z = 0, 1, 2
# ---- X/Y, fp32 ----------------------------------------------------------------------------------------------------------------
_c("xy-8ch-X-72", (72, 6, 33), X, 63, 16, (1, 16, 8, 32, 0, 1, 12), "chunk 4 half full, chunks 5-7 empty; dimz 33: a lone lane in the last tile")
_c("xy-8ch-Y-128", (6, 128, 8), Y, 111, 16, (1, 16, 8, 32, 0, 1, 6), "eight full chunks")
_c("xy-16ch-X-130", (130, 6, 8), X, 111, 16, (1, 16, 16, 32, 0, 1, 6), "two cells in chunk 8, chunks 9-15 empty")
_c("xy-16ch-Y-256", (8, 256, 33), Y, 127, 16, (1, 16, 16, 32, 0, 1, 16), "sixteen full chunks, a lone lane in the last tile")
_c("xy-32ch-X-260", (260, 6, 8), X, 255, 16, (1, 16, 32, 32, 0, 1, 6), "the register-light interface solve; plate at 255 | 256", fuses=(0, 1))
_c("xy-32ch-X-512", (512, 5, 33), X, 15, 16, (1, 16, 32, 32, 0, 1, 10), "32 full chunks; plate at 15 | 16; a lone lane", fuses=(0, 1))
_c("xy-32ch-Y-388", (6, 388, 8), Y, 255, 16, (1, 16, 32, 32, 0, 1, 6), "chunk 24 a quarter full; plate at 255 | 256", fuses=(0, 1))
_c("xy-32ch-Y-512", (6, 512, 8), Y, 15, 16, (1, 16, 32, 32, 0, 1, 6), "32 full chunks; plate at 15 | 16", fuses=(0, 1))
_c("xy-order0-X", (34, 512, 40), X, 15, 16, (1, 16, 4, 32, 0, 0, 1024), "1024 workgroups of 32-line tiles: consecutive ids walk the rows of one lane tile")
_c("xy-order0-Y", (512, 34, 40), Y, 15, 16, (1, 16, 4, 32, 0, 0, 1024), "the same for the Y kernel")
_c("xy-late-Y", (512, 130, 40), Y, 111, 16, (1, 16, 16, 32, 0, 0x440, 1024), "the late start: the default Y launch of a 256^3 box in small")
# ---- X/Y, fp64 ----------------------------------------------------------------------------------------------------------------
_c("xy64-8ch-X-72", (72, 6, 17), X, 63, 16, (1, 16, 8, 32, 0, 1, 6), "fp64, 32 lines x 8 chunks", dtype=F64)
_c("xy64-8ch-Y-72", (6, 72, 17), Y, 63, 16, (1, 16, 8, 32, 0, 1, 6), "the same for the Y kernel", dtype=F64)
_c("xy64-16ch-Y-130", (6, 130, 17), Y, 111, 16, (1, 16, 16, 16, 0, 1, 12), "fp64, 16-line tiles: dimz 17 leaves a lone lane in the second", dtype=F64)
_c("xy64-16ch-X-256", (256, 5, 8), X, 127, 16, (1, 16, 16, 16, 0, 1, 5), "fp64, sixteen full chunks, half a tile of lines", dtype=F64)
# ---- Z, fp32: 4 cells per lane ------------------------------------------------------------------------------------------------
_c("z-32-68", (6, 7, 68), Z, 63, 4, (2, 32, 1, 1, 4, 6), "17 of 32 lanes; 7 lines: the last row holds one of two")
_c("z-32-128", (6, 8, 128), Z, 63, 4, (2, 32, 1, 1, 4, 6), "32 full lanes")
_c("z-64-132", (6, 5, 132), Z, 127, 4, (2, 64, 1, 1, 5, 8), "33 of 64 lanes; 30 tasks: the last workgroup has two waves without one")
_c("z-64-256", (5, 6, 256), Z, 127, 4, (2, 64, 1, 1, 6, 8), "64 full lanes, what a 256^3 box runs")
_c("z-16-LG2", (512, 60, 8), Z, 3, 4, (2, 16, 1, 2, 8, 1024), "15 rows of 4 lines, two per wave: the last group holds one")
_c("z-16-LG4", (512, 118, 8), Z, 3, 4, (2, 16, 1, 4, 8, 1024), "30 rows: the last group holds two, the last row two lines past the plane")
_c("z-16-LG8", (512, 230, 8), Z, 3, 4, (2, 16, 1, 8, 8, 1024), "58 rows: the last group holds two, the last row two lines past the plane")
_c("z-16-LG16", (512, 450, 8), Z, 3, 4, (2, 16, 1, 16, 8, 1024), "113 rows: the last group holds one, the last row two lines past the plane")
_c("z-64-LG2", (64, 129, 132), Z, 127, 4, (2, 64, 1, 2, 65, 1040), "one line per wave-wide access, 129 rows: the last group holds one")
_c("z-pair-388", (8, 10, 388), Z, 255, 256, (2, 64, 2, 1, 10, 40), "END | START across the cut between the two waves of a line (cells 255 | 256)")
_c("z-pair-260", (7, 5, 260), Z, 251, 4, (2, 64, 2, 1, 5, 18), "35 tasks: the last workgroup's second pair is past the end; plate at the lower wave's last lane")
# ---- Z, fp64: 2 cells per lane ------------------------------------------------------------------------------------------------
_c("z64-16-26", (6, 7, 26), Z, 13, 2, (2, 16, 1, 1, 2, 3), "fp64, 13 of 16 lanes", dtype=F64)
_c("z64-64-66", (6, 5, 66), Z, 31, 2, (2, 64, 1, 1, 5, 8), "fp64, 33 of 64 lanes", dtype=F64)
_c("z64-64-128", (6, 6, 128), Z, 63, 2, (2, 64, 1, 1, 6, 9), "fp64, 64 full lanes", dtype=F64)
_c("z64-pair-130", (7, 5, 130), Z, 125, 2, (2, 64, 2, 1, 5, 18), "fp64, a pair of waves with one lane in the upper; 35 tasks", dtype=F64)
_c("z64-32-LG2", (512, 30, 34), Z, 15, 2, (2, 32, 1, 2, 8, 1024), "fp64, 15 rows of 2 lines, two per wave (two rows in flight)", dtype=F64)
# ---- x-slabs, 2 ranks: the slab sweep (XB 1) and the interface pass (XB 2) ------------------------------------------------------
_c("slab-4ch", (96, 20, 24), X, 47, 48, (1, 16, 4, 32, 1, 1, 20), "48-plane slabs, plate across the cut", ranks=2, record1=(1, 16, 4, 32, 2, 1, 20))
_c("slab-8ch", (160, 6, 24), X, 79, 80, (1, 16, 8, 32, 1, 1, 6), "80-plane slabs: five chunks", ranks=2, record1=(1, 16, 8, 32, 2, 1, 6))
_c("slab-16ch", (288, 6, 8), X, 143, 144, (1, 16, 16, 64, 1, 0, 6), "144-plane slabs: nine chunks", ranks=2, record1=(1, 16, 16, 64, 2, 0, 6))
_c("slab-4ch-wide", (96, 512, 8), X, 47, 48, (1, 16, 4, 64, 1, 0, 512), "dimy x ceil(dimz / 64) >= 512: 64-line tiles", ranks=2, record1=(1, 16, 4, 64, 2, 0, 512))
_c("slab-8ch-wide", (160, 512, 8), X, 79, 80, (1, 16, 8, 64, 1, 0, 512), "the same with 80-plane slabs", ranks=2, record1=(1, 16, 8, 64, 2, 0, 512))
# ---- the bc_cases grids that already hold a shape ---------------------------------------------------------------------------------
_bc("bc-F-A-X", "F-A", X, (1, 16, 4, 32, 0, 1, 100), "three chunks of 16, lane tiles fastest")
_bc("bc-F-A-Y", "F-A", Y, (1, 16, 4, 32, 0, 1, 68), "four chunks of 16")
_bc("bc-F-A-Z", "F-A", Z, (2, 16, 1, 1, 13, 111), "11 of 16 lanes, four lines per wave-wide access")
_bc("bc-W-X", "W-X", X, (1, 16, 16, 64, 0, 0, 512), "the 64-line X tiles of a 256^3 box")
_bc("bc-L-Z-260", "L-Z-260", Z, (2, 64, 2, 1, 6, 21), "a pair of waves, one lane in the upper")
_bc("bc-S-31", "S-31", X, (1, 8, 4, 64, 1, 0, 20), "32-plane slabs: 8-cell chunks", ranks=2, record1=(1, 8, 4, 64, 2, 0, 20))
_bc("bc64-F-A-X", "F-A", X, (1, 16, 4, 32, 0, 1, 100), "fp64, three chunks", dtype=F64)
_bc("bc64-F-A-Y", "F-A", Y, (1, 16, 4, 32, 0, 1, 68), "fp64, four chunks", dtype=F64)
_bc("bc64-F-A-Z", "F-A", Z, (2, 32, 1, 1, 25, 213), "fp64, 22 of 32 lanes, two lines per wave-wide access", dtype=F64)

NAMES = list(CASES)
MAX_DIM, MAX_CELLS = 512, 2700000


def instance(c):
    """The template instance an entry's record names: (precision, "xy", DIR, M, NCH, LT, XB) or (precision, "z", LPL, NW)."""
    p = np.dtype(c.dtype).name
    keys = [(p, "xy", c.d) + r[1:5] if r[0] == 1 else (p, "z") + r[1:3] for r in (c.record, c.record1) if r]
    return keys


def record_dict(rec):
    """A record as capi.Solver.last_sweep_launch returns it."""
    return {"family": 0} if rec is None else dict(zip(capi.Solver.LAUNCH_FIELDS[rec[0]], rec))


@functools.lru_cache(maxsize=None)
def _plates(dims, h, pos):
    g = BC.plates(dims, h, BC.face_kinds(BC.ASSIGN["B"]), BC.KINDS["FF"], pos)
    for a in (g.type, g.bc_vel, g.bc_temp, g.vx, g.vy, g.vz, g.T):
        a.setflags(write=False)
    return g


def grid(name):
    """The grid of that entry; shared, not to be written."""
    c = CASES[name]
    return BC.grid(c.grid) if c.grid else _plates(c.dims, c.h, c.pos)


def _grid_key(name):
    c = CASES[name]
    return c.grid or (c.dims, c.h, c.pos)


def seeded(name):
    """(cur, temp) of the seeded state in fp32; an fp64 context or oracle gets the same values."""
    return BC.seeded(CASES[name].grid) if CASES[name].grid else _seeded(_grid_key(name))


@functools.lru_cache(maxsize=2)
def _seeded(key):
    g = _plates(*key)
    base = [np.ascontiguousarray(a, np.float32) for a in (g.vx, g.vy, g.vz, g.T)]
    return BC._ro(grids.perturb(base, seed=1234)), BC._ro(grids.perturb(base, seed=1235))


def sweep_reference(name, dtype):
    """(next, merged temp) of ONE sweep of the entry's direction on the seeded state with `next` full of the sentinel, then
    next->MergeLayerTo(temp), by the CPU oracle in that precision."""
    return _sweep_reference(name if CASES[name].grid is None else CASES[name].grid, CASES[name].d, np.dtype(dtype))


@functools.lru_cache(maxsize=4)
def _sweep_reference(name, d, dtype):
    from oracle import oracle as O
    if name in BC.GRIDS:
        g, (cur, tmp) = BC.grid(name), BC.seeded(name)
    else:
        g, (cur, tmp) = grid(name), seeded(name)
    o = O.Oracle(g, capi.fluid_params(dtype.type, *BC.PARAMS), dtype.type)
    for v in range(4):
        o.set_field(O.L_CUR, v, cur[v].astype(o.dtype)); o.set_field(O.L_TEMP, v, tmp[v].astype(o.dtype))
        o.set_field(O.L_NEXT, v, np.full(o.dims, BC.SENTINEL, o.dtype))
    o.sweep(d, BC.DT, O.L_CUR, O.L_TEMP, O.L_NEXT)
    nxt = BC._ro(o.get_layer_fields(O.L_NEXT))
    o.merge(O.L_NEXT, O.L_TEMP)
    out = nxt, BC._ro(o.get_layer_fields(O.L_TEMP))
    o.close()
    return out
