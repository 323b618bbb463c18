"""Geometries that put every boundary-row kind into every sweep direction, and the CPU oracle's results on them, for
tests/test_bc_cases.py (CPU conditions) and tests/test_gpu_bc_matrix.py (the kernels).

A sweep kernel builds the first and the last row of a segment from a 4-bit row code: START or END, velocity BC NOSLIP or FREE,
temperature BC NOSLIP or FREE -- 8 codes per direction, 24 in all.  A kind is written as two letters, velocity first: "NN", "NF",
"FN", "FF" (N = NOSLIP, F = FREE).

faces_box: grids.box with the open part of each of the six faces a valve of its own kind.  The four assignments A-D form a Latin
square: over the four grids each kind is the START (low face) and the END (high face) row of every direction.
plates: a faces_box plus, per axis, two two-cell-thick plates (no NODE_OUT cell inside): a line through a plate has an END and a
START on adjacent cells.

The references (the CPU oracle in fp32 and in fp64 on the same seeded state) are computed once per process and handed out
read-only.
"""
import functools

import numpy as np

from cmc_fluid_solver_amd import capi, grids

DT = 0.1
PARAMS = (200.0, 0.72, 1.4)
SENTINEL = 7.25
KINDS = {"NN": (grids.BC_NOSLIP, grids.BC_NOSLIP), "NF": (grids.BC_NOSLIP, grids.BC_FREE),
         "FN": (grids.BC_FREE, grids.BC_NOSLIP), "FF": (grids.BC_FREE, grids.BC_FREE)}
SURFACE_V, SURFACE_T = (0.02, -0.03, 0.01), 1.1           # what a block's or a plate's surface carries
VALVE_SPEED = 0.3

# (low, high) kind per axis
ASSIGN = {"A": (("NN", "FF"), ("FN", "NF"), ("FF", "NN")),
          "B": (("FF", "FN"), ("NF", "FF"), ("FN", "NF")),
          "C": (("NF", "NN"), ("NN", "FN"), ("NF", "FF")),
          "D": (("FN", "NF"), ("FF", "NN"), ("NN", "FN"))}
BLOCK_KIND = {"A": "FF", "B": "FN", "C": "NF", "D": "NN"}
LOW_NN_HIGH_FF = (("NN", "FF"),) * 3


def face_kinds(assign):
    """{(axis, side): (bc_vel, bc_temp)} from three (low, high) pairs of kind names."""
    return {(ax, side): KINDS[assign[ax][side]] for ax in range(3) for side in range(2)}


def faces_box(dims, h, kinds, block=None):
    """grids.box with the open part of face (axis, side) a NODE_VALVE of kinds[(axis, side)] = (bc_vel, bc_temp).  A NOSLIP-velocity
    valve carries 0.3 along its axis; the faces of axis a have T = 1 - 0.05 (a + 1) (low) and 1 + 0.05 (a + 1) (high).
    block = ((lo, hi), (bc_vel, bc_temp)): a solid block over the cells lo .. hi (inclusive) whose one-cell surface is NODE_BOUND of
    that kind with non-zero values and whose inside is NODE_OUT."""
    g = grids.box(*dims, h=h)
    for ax in range(3):
        for side in range(2):
            bc_vel, bc_temp = kinds[(ax, side)]
            face = np.zeros(g.shape, bool)
            sel = [slice(1, -1)] * 3
            sel[ax] = -1 if side else 0
            face[tuple(sel)] = True
            v = [0.0, 0.0, 0.0]
            if bc_vel == grids.BC_NOSLIP:
                v[ax] = VALVE_SPEED
            grids._set_bound(g, face, bc_vel, bc_temp, tuple(v), 1.0 + (0.05 if side else -0.05) * (ax + 1), grids.NODE_VALVE)
    if block is not None:
        (lo, hi), (bc_vel, bc_temp) = block
        blk = np.zeros(g.shape, bool)
        blk[tuple(slice(a, b + 1) for a, b in zip(lo, hi))] = True
        inner = np.zeros(g.shape, bool)
        inner[tuple(slice(a + 1, b) for a, b in zip(lo, hi))] = True
        grids._set_bound(g, blk, bc_vel, bc_temp, SURFACE_V, SURFACE_T)
        g.type[inner] = grids.NODE_OUT
        g.bc_vel[inner] = grids.BC_NOSLIP
        g.bc_temp[inner] = grids.BC_NOSLIP
        g.vx[inner] = g.vy[inner] = g.vz[inner] = 0.0
        g.T[inner] = 0.0
    return g


def plates(dims, h, kinds, plate_kind, pos):
    """faces_box plus two plates per axis, two cells thick along it, of plate_kind: cells pos[ax], pos[ax] + 1 across 15-45 % of both
    cross directions, and cells 2, 3 (one NODE_IN cell off the low wall: a three-cell segment) across 55-85 %.  Only NODE_IN cells
    are carved."""
    g = faces_box(dims, h, kinds)
    fluid = g.type == grids.NODE_IN
    plate = np.zeros(g.shape, bool)
    for ax in range(3):
        for first, (a, b) in ((pos[ax], (0.15, 0.45)), (2, (0.55, 0.85))):
            sel = [slice(int(a * n), int(b * n)) for n in g.shape]
            sel[ax] = slice(first, first + 2)
            plate[tuple(sel)] = True
    grids._set_bound(g, plate & fluid, *plate_kind, SURFACE_V, SURFACE_T)
    return g


F_DIMS, F_LO, F_HI = (34, 50, 44), (16, 16, 20), (31, 31, 31)
P_POS = (15, 31, 19)
S_DIMS = (64, 20, 24)

GRIDS = {}
for _n in "ABCD":
    GRIDS["F-" + _n] = functools.partial(faces_box, F_DIMS, 0.03, face_kinds(ASSIGN[_n]), ((F_LO, F_HI), KINDS[BLOCK_KIND[_n]]))
for _k in ("FF", "FN", "NF", "NN"):
    GRIDS["P-" + _k] = functools.partial(plates, F_DIMS, 0.03, face_kinds(LOW_NN_HIGH_FF), KINDS[_k], P_POS)
GRIDS["L-Z-388"] = functools.partial(faces_box, (8, 10, 388), 0.003, face_kinds(ASSIGN["A"]))       # Z lines held by a pair of waves
GRIDS["L-Z-260"] = functools.partial(faces_box, (7, 6, 260), 0.004, face_kinds(ASSIGN["B"]))
GRIDS["W-X"] = functools.partial(faces_box, (130, 512, 8), 0.01, face_kinds(ASSIGN["B"]))           # the smallest grid on the 64-line X tiles
GRIDS["E-line"] = functools.partial(faces_box, (18, 22, 70), 0.03, face_kinds(ASSIGN["C"]),         # 70-cell Z lines: the exact kernels
                                    (((7, 8, 20), (12, 14, 41)), KINDS[BLOCK_KIND["C"]]))
GRIDS["S-31"] = functools.partial(plates, S_DIMS, 0.03, face_kinds(ASSIGN["D"]), KINDS["FF"], (31, 9, 11))   # END | START across the cut of 2 ranks
GRIDS["S-32"] = functools.partial(plates, S_DIMS, 0.03, face_kinds(ASSIGN["D"]), KINDS["FF"], (32, 9, 11))   # FREE END on the upper rank's first plane

F_GRIDS = ["F-A", "F-B", "F-C", "F-D"]
P_GRIDS = ["P-FF", "P-FN", "P-NF", "P-NN"]
L_GRIDS = ["L-Z-388", "L-Z-260"]
S_GRIDS = ["S-31", "S-32"]
# the sweep directions a test runs on a grid (the long or wide ones: the direction they are about)
DIRS = {n: (0, 1, 2) for n in GRIDS}
DIRS.update({"L-Z-388": (2,), "L-Z-260": (2,), "W-X": (0,)})


@functools.lru_cache(maxsize=None)
def grid(name):
    """The grid of that name; shared, not to be written."""
    g = GRIDS[name]()
    for a in (g.type, g.bc_vel, g.bc_temp, g.vx, g.vy, g.vz, g.T):
        a.setflags(write=False)
    return g


def row_codes(g, d):
    """The 4-bit row codes of direction d, [i][j][k], from the numpy restatement of the geometry tables."""
    import test_geom_tables as GT
    return (GT.restate(g)["code"].reshape(g.shape) >> (4 * d)) & 0xF


def code_name(code):
    return "SE"[(int(code) & 3) == 3] + ("v" if code & 4 else "-") + ("t" if code & 8 else "-")


# ---- the references -------------------------------------------------------------------------------------------------------

def _ro(fields):
    for a in fields:
        a.setflags(write=False)
    return fields


@functools.lru_cache(maxsize=None)
def seeded(name):
    """(cur, temp) of the seeded state in fp32; an fp64 context or oracle gets the same values."""
    g = grid(name)
    base = [np.ascontiguousarray(a, np.float32) for a in (g.vx, g.vy, g.vz, g.T)]
    return _ro(grids.perturb(base, seed=1234)), _ro(grids.perturb(base, seed=1235))


def _oracle(name, dtype):
    from oracle import oracle as O
    return O, O.Oracle(grid(name), capi.fluid_params(dtype, *PARAMS), dtype)


def _seed_oracle(O, o, name):
    cur, tmp = seeded(name)
    for v in range(4):
        o.set_field(O.L_CUR, v, cur[v].astype(o.dtype)); o.set_field(O.L_TEMP, v, tmp[v].astype(o.dtype))
        o.set_field(O.L_NEXT, v, np.full(o.dims, SENTINEL, o.dtype))


@functools.lru_cache(maxsize=None)
def sweep_reference(name, dtype):
    """{d: (next, merged temp)} of ONE sweep of direction d on the seeded state with `next` full of the sentinel, then
    next->MergeLayerTo(temp); every direction starts from the seeded state again."""
    O, o = _oracle(name, dtype)
    out = {}
    for d in DIRS[name]:
        _seed_oracle(O, o, name)
        o.sweep(d, DT, O.L_CUR, O.L_TEMP, O.L_NEXT)
        nxt = _ro(o.get_layer_fields(O.L_NEXT))
        o.merge(O.L_NEXT, O.L_TEMP)
        out[d] = (nxt, _ro(o.get_layer_fields(O.L_TEMP)))
    o.close()
    return out


@functools.lru_cache(maxsize=None)
def merged_run_reference(name, dtype, dirs=(0, 1, 2), steps=2):
    """One merged sweep per direction in turn on the seeded state (`next` starts full of the sentinel), then `steps` time steps
    (G 4, L 2): ([(next, temp) after each sweep], cur at the end, [divergence error per step], [rc per step])."""
    O, o = _oracle(name, dtype)
    _seed_oracle(O, o, name)
    sweeps, errs, rcs = [], [], []
    for d in dirs:
        o.sweep(d, DT, O.L_CUR, O.L_TEMP, O.L_NEXT); o.merge(O.L_NEXT, O.L_TEMP)
        sweeps.append((_ro(o.get_layer_fields(O.L_NEXT)), _ro(o.get_layer_fields(O.L_TEMP))))
    for _ in range(steps):
        o.update_boundaries()
        rc, e = o.time_step(DT, 4, 2, True)
        rcs.append(rc); errs.append(e)
    cur = _ro(o.get_layer_fields(O.L_CUR))
    o.close()
    return sweeps, cur, errs, rcs


@functools.lru_cache(maxsize=None)
def steps_reference(name, dtype, steps=3):
    """`steps` time steps (G 4, L 2) from the node state: ([cur after each step], [divergence error], [rc])."""
    O, o = _oracle(name, dtype)
    curs, errs, rcs = [], [], []
    for _ in range(steps):
        o.update_boundaries()
        rc, e = o.time_step(DT, 4, 2, True)
        curs.append(_ro(o.get_layer_fields(O.L_CUR))); errs.append(e); rcs.append(rc)
    o.close()
    return curs, errs, rcs


# ---- the per-line criterion -----------------------------------------------------------------------------------------------
# A rel-L2 norm over the whole grid hides rows that are wrong on one line at a tile edge.  Per field, over the cells the fp64 oracle
# wrote: S = max |x64|, e(K) = max over the lines of the sweep direction of max |K - x64| / S.  A kernel passes with
#     e(kernel) <= F e(oracle32) + 2^-23,
# oracle32 being the reference's own sequential fp32 arithmetic; the floor is one fp32 rounding of the field scale, which cannot be
# told from correct.  F = 2 comes from the numpy model of the kernels' chunkings (16-cell chunks with a sequential interface solve,
# 4-cell chunks with cyclic reduction), which tests/test_partition_algebra.py holds to the same criterion on two-segment lines
# with every end-row kind at every chunk offset: not from what the kernels give.
F_LINE = 2.0
FLOOR = 2.0 ** -23


def line_error(K, x64, written, d):
    """e(K) and the (o1, o2) index of the worst line of direction d."""
    x64 = np.asarray(x64, np.float64)
    S = np.abs(x64[written]).max()
    err = np.where(written, np.abs(np.asarray(K, np.float64) - x64), 0.0).max(axis=d) / S
    return float(err.max()), tuple(int(i) for i in np.unravel_index(err.argmax(), err.shape))


def check_lines(K, X32, X64, written, d, what, scale=1.0):
    """The criterion on four fields; `written` per field.  Prints both errors and returns the ratios e(kernel) / e(oracle32)."""
    ratios = []
    for v in range(4):
        ek, where = line_error(K[v], X64[v], written[v], d)
        eo, _ = line_error(X32[v], X64[v], written[v], d)
        bound = (F_LINE * eo + FLOOR) * scale
        print("%s field %d: per-line e(kernel) %.3e  e(oracle32) %.3e  ratio %.2f  bound %.3e  worst line %s" % (
            what, v, ek, eo, ek / (eo * scale), bound, where))
        assert np.isfinite(np.asarray(K[v])).all(), "%s: field %d has non-finite values" % (what, v)
        assert ek <= bound, "%s: field %d: worst line %s of direction %d is off by %.3e of the field scale > %.3e (oracle32: %.3e)" % (
            what, v, where, d, ek, bound, eo)
        ratios.append(ek / (eo * scale))
    return ratios
