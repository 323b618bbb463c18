"""No GPU: the fields of output_digest_cases.py can tell one order of summation from another, on the very boxes the pinned records
average.  Per case and precision: among the boxes with two or more NODE_IN cells, those whose double sum over the fluid cells
changes when the cells are added in reversed order are at least one third -- for each of the four fields.  A sum of two terms is
the same in either order whatever the terms are, so no field can meet that where most boxes are pairs: PAIRS -- the long thin
grid with its one fluid line, 292 pairs in 292 boxes, and 12 x 9 x 10 -> 20 x 4 x 7 with one plane per box, 225 pairs in 313 boxes and
none of more than four cells.  There the test asks that no pair differs and, where larger boxes exist, that some of them do.  Cases
of single cells have no sum; they are pinned for their bytes."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import output_digest_cases as DC  # noqa: E402
from cmc_fluid_solver_amd import grids  # noqa: E402
from cmc_fluid_solver_amd import layer_output as LO  # noqa: E402

PAIRS = [((3, 3, 600), (2, 2, 300)), ((12, 9, 10), (20, 4, 7))]
GEOMETRIES = sorted({(dims, od) for dims, od in DC.WHOLE} | {(dims, od) for dims, od, _ in DC.SLABS})


def serial_sum(x):
    return float(np.cumsum(x)[-1])                         # cumsum adds one after the other (np.sum adds in pairs)


@pytest.mark.parametrize("dtype", DC.DTYPES, ids=DC.name)
def test_values_are_exact_and_spread_over_the_binades(dtype):
    f = DC.hashed_fields((23, 13, 11), dtype, 1)           # (hashed_fields asserts the exactness itself)
    g = DC.hashed_fields((23, 13, 11), dtype, 2)
    assert all(a.dtype == np.dtype(dtype) and np.isfinite(a).all() for a in f)
    assert not any(np.array_equal(a, b) for a, b in zip(f, g)), "the salt changes the fields"
    for a in f:
        e = np.frexp(a.astype(np.float64))[1]
        assert len(np.unique(e)) == 2 * DC.JITTER and np.ptp(e) == DC.GAP + DC.JITTER - 1 and (a < 0).any() and (a > 0).any()
        m = np.abs(np.ldexp(a.astype(np.float64), 24 - e)).astype(np.int64) if dtype == np.float32 else None
        assert m is None or (m % 2 == 1).all(), "odd 24-bit mantissas"


@pytest.mark.parametrize("dtype", DC.DTYPES, ids=DC.name)
def test_a_reversed_sum_differs_in_a_third_of_the_boxes(dtype):
    asked = 0
    for dims, od in GEOMETRIES:
        fluid = DC.nodes_of(dims).type == grids.NODE_IN
        ax = [LO.boxes(g, o) for g, o in zip(dims, od)]
        for salt in (1, 2):
            fields = [f.astype(np.float64) for f in DC.hashed_fields(dims, dtype, salt)]
            boxes, three, differ = 0, 0, [0, 0, 0, 0]
            for x0, x1 in zip(*ax[0]):
                for y0, y1 in zip(*ax[1]):
                    for z0, z1 in zip(*ax[2]):
                        box = (slice(x0, x1), slice(y0, y1), slice(z0, z1))
                        m = fluid[box]
                        n = int(m.sum())
                        if n < 2:
                            continue
                        boxes += 1
                        three += n >= 3
                        for v in range(4):
                            q = fields[v][box][m]
                            differ[v] += serial_sum(q) != serial_sum(q[::-1])
            print("%s -> %s %s salt %d: %d boxes of two or more fluid cells (%d of three or more), reversed sum differs in %s" %
                  (dims, od, DC.name(dtype), salt, boxes, three, differ))
            assert ((dims, od) in PAIRS) == (boxes > 0 and 3 * three < boxes), "PAIRS lists the cases whose boxes are mostly pairs"
            asked += boxes > 0
            if (dims, od) in PAIRS:
                assert all(d <= three and (d > 0) == (three > 0) for d in differ), (dims, od, salt, boxes, three, differ)
            else:
                assert all(3 * d >= boxes for d in differ), (dims, od, salt, boxes, three, differ)
    assert asked == 2 * 8, "both field sets on the eight cases that have boxes"
