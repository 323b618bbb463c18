"""Fresh cells of a moving geometry: what a cell holds when a wall moves off it and it becomes NODE_IN.

fill_fresh_cells is the definition of the rule; fs3d_fill_fresh_cells / fs3d_fill_fresh_cells_dev (csrc/kernels_geom.hip:
k_fresh_classify, k_fresh_round) are held to it bit for bit.  The reference has no counterpart: it never moves a 3D geometry
between steps.

With prev_type the node types before the geometry update and type the ones after it, every cell is one of
  donor   type == NODE_IN and prev_type == NODE_IN
  fresh   type == NODE_IN and prev_type != NODE_IN
  other   everything else: never read, never written.
The fill runs in rounds r = 1, 2, ...  Every fresh cell still unfilled at the start of round r looks at its six neighbours in the
fixed order i-1, i+1, j-1, j+1, k-1, k+1 (outside the grid: skipped); a neighbour counts if it is a donor or was filled in a round
before r.  With n >= 1 counting neighbours each of the four fields becomes (x1 + x2 + .. + xn) / (R)n -- the first value starts the
sum, the others are added in that order, every addition and the one division rounded in R, the precision of the fields -- and the
cell is filled in round r.  A round reads only the state before the round, so the order in which cells are visited is free.  The
fill stops after the first round that fills nothing, or after max_rounds rounds.  Fresh cells that no chain of fresh cells joins
to a donor keep what they hold.  Every filled value lies between the smallest and the largest donor value of its field (a mean of
values in an interval, rounded monotonically, stays in it).
"""
import numpy as np

from .grids import NODE_IN

MAX_ROUNDS = 250
NEIGHBOURS = ((0, -1), (0, 1), (1, -1), (1, 1), (2, -1), (2, 1))       # (axis, step): i-1, i+1, j-1, j+1, k-1, k+1


def classes(prev_type, type):
    """(donor, fresh) as boolean arrays"""
    now = np.asarray(type) == NODE_IN
    was = np.asarray(prev_type) == NODE_IN
    return now & was, now & ~was


def fill_fresh_cells(prev_type, type, fields, max_rounds=0, order=None):
    """fields: u, v, w, T of one layer, four arrays [dimx, dimy, dimz] of one float dtype (not modified).
    order: the flat indices of the fresh cells in the order they are to be visited in every round (default: ascending); the result
    does not depend on it.
    Returns (the four filled arrays, (fresh, filled, rounds, fresh - filled)); rounds counts those that filled at least one cell."""
    if not 0 <= max_rounds <= MAX_ROUNDS:
        raise ValueError("max_rounds is 0 .. %d (0: %d)" % (MAX_ROUNDS, MAX_ROUNDS))
    limit = max_rounds or MAX_ROUNDS
    out = [np.array(f, copy=True) for f in fields]
    R = out[0].dtype.type
    if any(f.dtype != out[0].dtype or f.dtype.kind != "f" for f in out):
        raise ValueError("four fields of one float dtype")
    dims = out[0].shape
    donor, fresh = classes(prev_type, type)
    if donor.shape != dims:
        raise ValueError("the types do not have the fields' shape")
    ok = donor.copy()                                     # cells a neighbour may read: donors, and what earlier rounds filled
    todo = np.flatnonzero(fresh) if order is None else np.asarray(order, np.int64).reshape(-1)
    if order is not None and not np.array_equal(np.sort(todo), np.flatnonzero(fresh)):
        raise ValueError("order lists every fresh cell once")
    n_fresh, filled, rounds = int(fresh.sum()), 0, 0
    for r in range(1, limit + 1):
        done = []                                         # (cell, four values): written after the round, which reads the state before it
        for l in todo:
            c = np.unravel_index(l, dims)
            n, s = 0, None
            for axis, step in NEIGHBOURS:
                m = list(c)
                m[axis] += step
                if not 0 <= m[axis] < dims[axis] or not ok[tuple(m)]:
                    continue
                x = [f[tuple(m)] for f in out]
                s = x if n == 0 else [a + b for a, b in zip(s, x)]
                n += 1
            if n:
                done.append((c, [a / R(n) for a in s]))
        if not done:
            break
        for c, vals in done:
            for f, x in zip(out, vals):
                f[c] = x
            ok[c] = True
        was_done = set(int(np.ravel_multi_index(c, dims)) for c, _ in done)
        todo = np.array([l for l in todo if int(l) not in was_done], np.int64)
        filled += len(done)
        rounds += 1
        if filled == n_fresh:
            break
    return out, (n_fresh, filled, rounds, n_fresh - filled)
