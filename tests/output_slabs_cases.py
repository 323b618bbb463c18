"""The cases of the filtered and derived result records on x-slabs (FS3D_OPT_OUTPUT_SLABS), shared by the CPU test of the numpy
twin (test_output_slabs_cases.py) and the GPU test of the library (test_gpu_output_slabs.py).

A case is (global grid, output dims, ranks); the slabs are slab.slab_range's.  STRADDLING holds, per case, the rows whose box
holds planes of more than one slab -- worked out by hand from lo = i*g // o, hi = max(lo + 1, (i+1)*g // o):
  23 -> 5: boxes [0,4) [4,9) [9,13) [13,18) [18,23); 2 slabs cut at 12, 3 slabs at 8 and 16, 4 slabs at 6, 12 and 18 (a cut at a
           box edge, 18, crosses no box);
  13 -> 2: boxes [0,6) [6,13); cuts at 4, 7, 10 -- row 1 holds planes of the ranks 1, 2 and 3, and the ranks 2 and 3 own no row;
   6 -> 1: one box over every slab;
  13 -> 13 and 12 -> 20: single-cell boxes, none straddles -- only the curl crosses the cuts."""
import numpy as np

from cmc_fluid_solver_amd import layer_output as LO
from cmc_fluid_solver_amd.slab import slab_range

MODES = [(1, 0), (0, 1), (1, 1)]                                    # (filter, vector)
POW2 = (0.25, 0.125, 0.5)
GENERAL = (0.3, 0.07, 0.11)
CASES = [((23, 13, 11), (5, 4, 7), 2), ((23, 13, 11), (5, 4, 7), 3), ((23, 13, 11), (5, 4, 7), 4),
         ((13, 11, 10), (2, 3, 4), 4),
         ((13, 11, 10), (0, 0, 0), 3),
         ((12, 9, 10), (20, 4, 7), 3),
         ((6, 5, 130), (1, 2, 40), 3)]
STRADDLING = [[2], [1, 3], [1, 2], [0, 1], [], [], [0]]


def case_id(case):
    dims, od, nranks = case
    return "%s-to-%s-on-%d" % ("x".join(map(str, dims)), "x".join(map(str, od)), nranks)


def cuts_of(gx, nranks):
    return [slab_range(gx, r, nranks) for r in range(nranks)]


def own(a, cut):
    return np.ascontiguousarray(a[cut[0]:cut[1]])


def rows_at_cuts(cuts, gx, odx):
    """The rows of the record that a cut can change: those whose box holds a plane next to a cut"""
    lo, hi = LO.boxes(gx, odx)
    rows = set()
    for x0, _ in cuts[1:]:
        rows |= {int(i) for i in np.nonzero((lo <= x0) & (hi > x0 - 1))[0]}
    return sorted(rows)


def naive_record(type, fields, cuts, outdims, filter, vector, spacing):
    """What the slabs would write without a word to each other: every slab runs the rule on its own planes as if they were the
    grid -- the boxes of its rows clipped at the cuts, the curl zero on a cut's planes (a neighbour is outside its grid)."""
    type = np.asarray(type)
    ax = [LO.boxes(g, o) for g, o in zip(type.shape, outdims)]
    od = [len(lo) for lo, _ in ax]
    outV, outT = None, np.full(od, np.nan, np.float64)
    for rank, (xs0, xs1) in enumerate(cuts):
        t = type[xs0:xs1]
        q = LO.cell_quantities(t, [f[xs0:xs1] for f in fields], vector, spacing)
        if outV is None:
            outV = np.full(od + [3], np.nan, q[0].dtype)
        fluid = t == LO.NODE_IN
        i0, i1 = LO.owned_rows(cuts, rank, type.shape[0], od[0])
        for i in range(i0, i1):
            x0, x1 = int(ax[0][0][i]) - xs0, min(int(ax[0][1][i]), xs1) - xs0
            for j, (y0, y1) in enumerate(zip(*ax[1])):
                for k, (z0, z1) in enumerate(zip(*ax[2])):
                    box = (slice(x0, x1), slice(y0, y1), slice(z0, z1))
                    m = fluid[box] if filter else np.zeros(fluid[box].shape, bool)
                    n = int(m.sum())
                    if n:
                        mean = [float(f[box][m].astype(np.float64).sum()) / n for f in q]
                        outV[i, j, k] = np.array(mean[:3]).astype(q[0].dtype)
                        outT[i, j, k] = mean[3]
                    else:
                        outV[i, j, k] = [f[x0, y0, z0] for f in q[:3]]
                        outT[i, j, k] = np.float64(q[3][x0, y0, z0])
    return outV, outT
