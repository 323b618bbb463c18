"""The local row-kind rule of the geometry tables (kernels_geom.hip, fs3d_tables.h), restated with whole-array operations for the
tests that hold the tables to it."""
import numpy as np

from cmc_fluid_solver_amd import grids

ROW_SKIP, ROW_INTERIOR, ROW_START, ROW_END = 0, 1, 2, 3


def rule_masks(type3, d):
    """The local rule along axis d, which is moved last: with Lst = the last index of a line whose type is not NODE_IN, cell s is
    INTERIOR iff s >= 1, its type is NODE_IN and s < Lst; START iff s + 1 is INTERIOR and s is not; END iff s is not INTERIOR and
    s - 1 is.  Returns the three masks (a cell that closes one segment and opens the next is in both START and END)."""
    ty = np.moveaxis(type3, d, 2)
    n = ty.shape[2]
    notin = ty != grids.NODE_IN
    s = np.arange(n)
    lst = np.where(notin, s, -1).max(axis=2)
    interior = (~notin) & (s >= 1) & (s < lst[..., None])
    nxt = np.zeros_like(interior); nxt[..., :-1] = interior[..., 1:]
    prv = np.zeros_like(interior); prv[..., 1:] = interior[..., :-1]
    return interior, ~interior & nxt, ~interior & prv


def rule_segments(type3, d):
    """The segments of the local rule (rule_masks) as the set of (start cell, end cell) index triples: the starts and the ends of a
    line pair up in order."""
    _, start, end = rule_masks(type3, d)
    a, b = np.argwhere(start), np.argwhere(end)          # both sorted by (line, s)
    assert len(a) == len(b) and np.array_equal(a[:, :2], b[:, :2]) and (a[:, 2] < b[:, 2]).all()
    inv = {0: (2, 0, 1), 1: (0, 2, 1), 2: (0, 1, 2)}[d]   # moved axes back to (i, j, k)
    return {(tuple(int(p[q]) for q in inv), tuple(int(e[q]) for q in inv)) for p, e in zip(a, b)}


def rule_kinds(type3, d):
    """Row kind per cell, indexed (i, j, k): START wins on a cell that closes one segment and opens the next, so the START cells
    count the segments.  Also the mask of those shared cells."""
    interior, start, end = rule_masks(type3, d)
    kind = np.where(interior, ROW_INTERIOR, np.where(start, ROW_START, np.where(end, ROW_END, ROW_SKIP))).astype(np.uint16)
    return np.ascontiguousarray(np.moveaxis(kind, 2, d)), np.ascontiguousarray(np.moveaxis(start & end, 2, d))
