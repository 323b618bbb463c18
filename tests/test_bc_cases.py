"""CPU conditions of the boundary-row grids of tests/bc_cases.py: what tests/test_gpu_bc_matrix.py takes for granted before it
blames a kernel.  Every grid builds (no shared FREE cell, no stale NODE_IN cell, the oracle's segment counts); the four F grids
together hold all 24 row codes; the END and START rows sit on the chunk and lane edges they are placed for; the CPU oracle is
finite on the seeded state and walks three steps; and the reference's own fp32 arithmetic leaves the 1.5 x yardstick of
tests/test_gpu_part.py room under its 5e-6 cap."""
import numpy as np
import pytest

import bc_cases as BC
import test_geom_tables as GT
from geom_rules import ROW_END, ROW_START

ALL = list(BC.GRIDS)


def rel(a, b):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


@pytest.mark.parametrize("name", ALL)
def test_grid_builds_like_the_oracle(built, name):
    g = BC.grid(name)
    t = GT.restate(g)
    assert t["shared_free"] is False and t["stale_in_cells"] == 0
    assert t["nseg"] == GT.oracle_nseg(g)


def test_f_grids_hold_all_24_row_codes(built):
    seen = {}
    for name in BC.F_GRIDS:
        g = BC.grid(name)
        for d in range(3):
            codes = BC.row_codes(g, d)
            ends = codes[((codes & 3) == ROW_START) | ((codes & 3) == ROW_END)]
            for c in np.unique(ends):
                seen.setdefault((d, int(c)), []).append(name)
    want = {(d, kind | vf | tf) for d in range(3) for kind in (ROW_START, ROW_END) for vf in (0, GT.ROW_VELFREE) for tf in (0, GT.ROW_TEMPFREE)}
    for d in range(3):
        print("XYZ"[d], sorted(BC.code_name(c) for dd, c in seen if dd == d))
    assert len(want) == 24 and set(seen) == want, sorted(want - set(seen))


def _line(codes, d, at):
    """the codes along direction d through the cell `at`"""
    sel = list(at)
    sel[d] = slice(None)
    return codes[tuple(sel)]


@pytest.mark.parametrize("name", BC.F_GRIDS)
def test_f_grid_block_rows_sit_on_chunk_and_lane_edges(built, name):
    """The line through the middle of the block: its END row on the first cell of an X/Y chunk (16) or of a Z lane (20 = 0 mod 4),
    its START row on the last one (31 = 15 mod 16 = 3 mod 4), both of the block's kind."""
    g = BC.grid(name)
    bv, bt = BC.KINDS[BC.BLOCK_KIND[name[-1]]]
    bits = bv * GT.ROW_VELFREE | bt * GT.ROW_TEMPFREE
    mid = [(a + b) // 2 for a, b in zip(BC.F_LO, BC.F_HI)]
    for d in range(3):
        line = _line(BC.row_codes(g, d), d, mid)
        assert line[BC.F_LO[d]] == ROW_END | bits and line[BC.F_HI[d]] == ROW_START | bits
        assert not line[BC.F_LO[d] + 1:BC.F_HI[d]].any()
    assert BC.F_LO[0] % 16 == 0 and BC.F_LO[1] % 16 == 0 and BC.F_LO[2] % 4 == 0
    assert BC.F_HI[0] % 16 == 15 and BC.F_HI[1] % 16 == 15 and BC.F_HI[2] % 4 == 3


@pytest.mark.parametrize("name", BC.P_GRIDS + BC.S_GRIDS)
def test_plate_rows_sit_on_adjacent_cells(built, name):
    """A line through the plate at pos: END at pos, START at pos + 1, both of the plate's kind; through the plate by the low wall:
    a three-cell segment 0 .. 2 and a START at 3."""
    g = BC.grid(name)
    pos = BC.GRIDS[name].args[4]
    bv, bt = BC.GRIDS[name].args[3]
    bits = bv * GT.ROW_VELFREE | bt * GT.ROW_TEMPFREE
    for d in range(3):
        codes = BC.row_codes(g, d)
        at = [int(0.3 * n) for n in g.shape]
        line = _line(codes, d, at)
        assert line[pos[d]] == ROW_END | bits and line[pos[d] + 1] == ROW_START | bits, (d, [BC.code_name(c) for c in line[pos[d]:pos[d] + 2]])
        at = [int(0.7 * n) for n in g.shape]
        line = _line(codes, d, at)
        assert (line[0] & 3) == ROW_START and line[2] == ROW_END | bits and line[3] == ROW_START | bits


@pytest.mark.parametrize("name", ALL)
def test_oracle_is_finite_after_one_sweep_per_direction(built, name):
    for dtype in (np.float32, np.float64):
        for d, (nxt, tmp) in BC.sweep_reference(name, dtype).items():
            for v in range(4):
                assert np.isfinite(nxt[v]).all() and np.isfinite(tmp[v]).all(), (np.dtype(dtype).name, d, v)
                assert (nxt[v] != BC.SENTINEL).any()
    # both precisions wrote the same cells
    a, b = BC.sweep_reference(name, np.float32), BC.sweep_reference(name, np.float64)
    for d in a:
        for v in range(4):
            assert np.array_equal(a[d][0][v] == BC.SENTINEL, b[d][0][v] == BC.SENTINEL)


@pytest.mark.parametrize("name", BC.F_GRIDS + BC.P_GRIDS)
def test_oracle_walks_three_steps(built, name):
    """time_step returns 0 in both precisions, and the fp32 oracle stays close enough to the fp64 one for the yardstick of
    tests/test_gpu_part.py (1.5 x its deviation + 1e-7, and <= 5e-6) to be satisfiable: (5e-6 - 1e-7) / 1.5 = 3.26e-6."""
    c32, e32, rc32 = BC.steps_reference(name, np.float32)
    c64, e64, rc64 = BC.steps_reference(name, np.float64)
    assert rc32 == [0, 0, 0] and rc64 == [0, 0, 0]
    for step in range(3):
        for v in range(4):
            assert np.isfinite(c32[step][v]).all() and np.isfinite(c64[step][v]).all()
        num = sum(np.linalg.norm(a.astype(np.float64) - b) ** 2 for a, b in zip(c32[step][:3], c64[step][:3]))
        den = sum(np.linalg.norm(b) ** 2 for b in c64[step][:3])
        rv, rt = float(np.sqrt(num / den)), rel(c32[step][3], c64[step][3])
        print("%s step %d: fp32 oracle vs fp64 oracle: velocity %.2e, T %.2e, components %s; divergence error %.3e" % (
            name, step, rv, rt, ["%.1e" % rel(a, b) for a, b in zip(c32[step][:3], c64[step][:3])], e64[step]))
        assert rv <= 3.26e-6 and rt <= 3.26e-6
