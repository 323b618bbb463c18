"""The cases of tests/slab_geometry_cases.py, held on a CPU to the host definition of the tables (build_geom_tables through
tests/geom_tables_test.cpp): each one has the property the GPU test relies on."""
import numpy as np
import pytest

import slab_geometry_cases as SC
from cmc_fluid_solver_amd import grids
from test_geom_tables import program, run_builder  # noqa: F401  (program: a fixture)


@pytest.mark.parametrize("nranks", [2, 3, 4])
def test_solid_from_has_live_x_pieces_without_fluid(program, tmp_path, nranks):
    """Slab 1 holds the END cell of every X line through the fluid and no NODE_IN cell: live by the tables' definition, dead by
    the shortcut "no NODE_IN cell" that a whole line allows."""
    _, B = SC.pair("solid_from", nranks)
    x0, x1 = SC.ranges(B.dimx, nranks)[1]
    t = run_builder(program, tmp_path, B, x0, x1 - x0)
    assert not (B.type[x0:x1] == grids.NODE_IN).any()
    assert int(t["dead0"].sum()) == B.dimy * B.dimz - (B.dimy - 2) * (B.dimz - 2)
    shortcut = ~(B.type[x0:x1] == grids.NODE_IN).any(axis=0).reshape(-1)
    assert shortcut.all() and int((shortcut != t["dead0"].astype(bool)).sum()) == (B.dimy - 2) * (B.dimz - 2)


@pytest.mark.parametrize("name", ["obstacle", "obstacle2"])
def test_the_moved_block_lies_across_cuts(name):
    A, B = SC.pair(name)
    assert not np.array_equal(A.type, B.type)
    wall = np.flatnonzero((B.type[:, B.dimy // 2, B.dimz // 2] != grids.NODE_IN))[1:-1]      # the block's planes on the centre line
    cuts = {x0 for n in (2, 3, 4) for x0, _ in SC.ranges(B.dimx, n)[1:]}
    inside = {c for c in cuts if wall[0] < c <= wall[-1]}
    edge = {c for c in cuts if c == wall[-1] + 1}
    assert inside >= {15, 16} and (edge or 20 in inside), (wall, sorted(cuts))


@pytest.mark.parametrize("name", SC.OPEN)
def test_open_pairs_have_stale_cells_on_every_rank_count(program, tmp_path, name):
    A, B = SC.pair(name)
    assert run_builder(program, tmp_path, A)["stale_in_cells"] == 0
    for nranks in (2, 3, 4):
        assert sum(run_builder(program, tmp_path, B, x0, x1 - x0)["stale_in_cells"] for x0, x1 in SC.ranges(B.dimx, nranks)) > 0


def test_the_baffles_are_refused_where_the_gpu_test_says(program, tmp_path):
    for g, refusing in ((SC.baffle_x(), {0, 1, 2}), (SC.baffle_y(), {1})):
        got = {r for r, (x0, x1) in enumerate(SC.ranges(g.dimx, 3)) if run_builder(program, tmp_path, g, x0, x1 - x0)["shared_free"]}
        assert got == refusing
