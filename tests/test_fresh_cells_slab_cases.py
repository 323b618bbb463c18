"""CPU: the cases of tests/fresh_cells_cases.py cut into x-slabs (slab.slab_range).  The condition that keeps
tests/test_gpu_fresh_cells_slabs.py from passing for the wrong reason: a fill that every slab runs on its own, as if its cuts were
the grid's faces, must DIFFER from the fill of the global grid on the cases those tests call "across the cut" -- else a group that
never exchanged a plane would pass them.  The twin cmc_fluid_solver_amd.fresh_cells.fill_fresh_cells is the only code under test."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import fresh_cells_cases as FC  # noqa: E402
from cmc_fluid_solver_amd import fresh_cells, slab  # noqa: E402

RANKS = (2, 3, 4)
SEED = 11
# the cases whose fill crosses a cut, and where: (case, size) -> the numbers of ranks at which the slab-local fill differs
ACROSS = {
    ("thick-one", "12x10x16"): (2, 3, 4), ("thick-one", "9x7x11"): (2, 3, 4),
    ("thick-both", "12x10x16"): (2, 3, 4), ("thick-both", "9x7x11"): (2, 3, 4),
    ("capped", "12x10x16"): (2, 4), ("capped", "9x7x11"): (2, 3, 4),
    ("one-layer-x", "12x10x16"): (2, 4),
    ("mixed-origin", "12x10x16"): (2, 4), ("mixed-origin", "9x7x11"): (3, 4),
}


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


def ranges(dimx, nranks):
    return [slab.slab_range(dimx, r, nranks) for r in range(nranks)]


def local_fill(case, size, nranks, dtype=np.float32):
    """every slab filled on its own, its cuts taken for faces of the grid: (the four fields put together again, the infos)"""
    a, b = FC.pair(case, size)
    seeded = FC.fields(size, dtype, SEED)
    parts, infos = [], []
    for x0, x1 in ranges(a.type.shape[0], nranks):
        out, info = fresh_cells.fill_fresh_cells(a.type[x0:x1], b.type[x0:x1], [f[x0:x1] for f in seeded], FC.MAX_ROUNDS.get(case, 0))
        parts.append(out)
        infos.append(info)
    return [np.concatenate([p[v] for p in parts], axis=0) for v in range(4)], infos


def differing(case, size, nranks):
    want, _ = FC.expected(case, size, np.float32, SEED)
    got, _ = local_fill(case, size, nranks)
    return sum(int((bits(x) != bits(y)).sum()) for x, y in zip(got, want))


def test_the_cuts_partition_the_planes_and_the_small_grid_has_slabs_of_two_planes():
    for size, dims in FC.SIZES.items():
        for n in RANKS:
            r = ranges(dims[0], n)
            assert r[0][0] == 0 and r[-1][1] == dims[0] and all(r[q][1] == r[q + 1][0] for q in range(n - 1))
    assert ranges(9, 4) == [(0, 3), (3, 5), (5, 7), (7, 9)]
    assert ranges(12, 4) == [(0, 3), (3, 6), (6, 9), (9, 12)]


@pytest.mark.parametrize("case,size", list(ACROSS))
def test_a_fill_that_stops_at_the_cuts_differs_from_the_global_fill(case, size):
    counts = {n: differing(case, size, n) for n in RANKS}
    print(case, size, "differing field values at 2 / 3 / 4 ranks:", " / ".join(str(counts[n]) for n in RANKS))
    for n in RANKS:
        if n in ACROSS[(case, size)]:
            assert counts[n] > 0, (case, size, n)


@pytest.mark.parametrize("size", list(FC.SIZES))
@pytest.mark.parametrize("case", FC.CASES)
def test_every_case_is_counted(case, size):
    """the table of all cases, for the record: which ones a cut changes at all"""
    counts = [differing(case, size, n) for n in RANKS]
    print("%-14s %-9s %s" % (case, size, " / ".join(map(str, counts))))
    if case == "none":
        assert counts == [0, 0, 0]


def test_thick_one_at_four_ranks_is_a_chain_through_three_slabs():
    """12x10x16, planes 0-2 | 3-5 | 6-8 | 9-11: the wall i = 1 .. 5 goes, the fluid that was there before begins at i = 6 -- the
    donors stand on the third slab, the fill walks down through the second into the first in 5 rounds, and the last slab holds no
    fresh cell at all and still has to take part."""
    a, b = FC.pair("thick-one", "12x10x16")
    donor, fresh = fresh_cells.classes(a.type, b.type)
    r = ranges(12, 4)
    assert FC.expected("thick-one", "12x10x16", np.float32, SEED)[1][2] == 5
    per_slab = [int(fresh[x0:x1].sum()) for x0, x1 in r]
    print("fresh cells per slab:", per_slab)
    assert per_slab[0] > 0 and per_slab[1] > 0 and per_slab[2] == 0 and per_slab[3] == 0
    assert not donor[:r[2][0]].any() and donor[r[2][0]:r[2][1]].any()          # no donor before the third slab
    # the round that fills plane i is 6 - i: the first slab's planes 1, 2 wait for rounds 5, 4, past the second slab's 3, 2, 1
    _, infos = local_fill("thick-one", "12x10x16", 4)
    assert infos[0][1] == 0 and infos[1][1] == 0                                # on their own the two slabs fill nothing
